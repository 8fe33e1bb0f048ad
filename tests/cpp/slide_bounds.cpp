// The constants tests/slide_cases.py restates, printed from the headers themselves: "span L ring_pages max_span" for
// every length and ring, "width L W", "exp min max", "page cols".
#include <cstdio>

#include "csr_rowrec.hpp"
#include "csr_valpack.hpp"

int main() {
    const int lengths[3] = {12, 14, 16};
    for (int L : lengths) {
        static_assert(spal::rowrec_length_ok(12) && spal::rowrec_length_ok(14) && spal::rowrec_length_ok(16), "the lengths");
        for (unsigned pages = 0; pages <= 255; ++pages) printf("span %d %u %u\n", L, pages, spal::rowrec_max_span(L, pages * 256u));
        printf("width %d %d\n", L, spal::valpack_width(L));
    }
    printf("exp %d %d\n", spal::kValpackMinExp, spal::kValpackMaxExp);
    printf("high_bits %d\n", spal::kRowrecHighBits);
    return 0;
}

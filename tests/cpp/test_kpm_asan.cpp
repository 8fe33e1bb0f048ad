// test_kpm_asan.cpp -- the host half of the KPM moments (spalinalg_amd/csrc/kpm_host.hpp) as a stand-alone program under
// -fsanitize=address,undefined: the probe hash on exact-size buffers with a leading dimension, every refusal in the
// text's order, the interval's scalars, the column tile, the chunk and the scratch layout.  No library, no device.
#include "kpm_host.hpp"

#include <cstdio>
#include <cstdlib>
#include <vector>

using namespace spal;

#define CHECK(cond)                                                          \
    do {                                                                     \
        if (!(cond)) {                                                       \
            std::printf("FAILED %s:%d: %s\n", __FILE__, __LINE__, #cond);    \
            return 1;                                                        \
        }                                                                    \
    } while (0)

template <typename T>
static int probes() {
    CHECK(kpm_mix32(0) == 0u && kpm_mix32(1) == 1753845952u && kpm_mix32(2) == 3507691905u && kpm_mix32(3) == 1408362973u);
    const uint64_t n = 37, k = 5, ldz = 7;
    std::vector<T> z(n * ldz - (ldz - k), T(9));   // exactly up to the last read element: one more is out of bounds
    kpm_probes<T>(n, k, 11, z.data(), ldz);
    long sum = 0;
    for (uint64_t i = 0; i < n; ++i) {
        for (uint64_t j = 0; j < k; ++j) {
            CHECK(z[i * ldz + j] == T(1) || z[i * ldz + j] == T(-1));
            CHECK(z[i * ldz + j] == (T)kpm_probe_sign(i, j, 11));
            sum += (long)z[i * ldz + j];
        }
        for (uint64_t j = k; j < ldz && i + 1 < n; ++j) CHECK(z[i * ldz + j] == T(9));   // the padding stays
    }
    CHECK(sum > -(long)(n * k) / 2 && sum < (long)(n * k) / 2);
    CHECK(kpm_probe_sign(3, 2, (1ull << 32) + 7) == kpm_probe_sign(3, 2, 7));   // only seed mod 2^32 enters
    CHECK(kpm_probe_sign(0xffffffffull, 0xff, 0xffffffffffffffffull) * kpm_probe_sign(0xffffffffull, 0xff, 0xffffffffffffffffull) == 1);
    return 0;
}

static int refusals() {
    const double inf = std::numeric_limits<double>::infinity(), nan = std::numeric_limits<double>::quiet_NaN();
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_OK);
    CHECK(kpm_check(3, 2, 8, true, 10, 2, 10, 1, nan, nan) == KPM_OK);   // automatic: lo and hi are not looked at
    CHECK(kpm_check(0, 2, 2, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_DEGREE);
    CHECK(kpm_check(4097, 2, 8196, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_DEGREE);
    CHECK(kpm_check(4096, 256, 4097ull * 256, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_OK);
    CHECK(kpm_check(3, 0, 0, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_PROBES);
    CHECK(kpm_check(3, 257, 4 * 257, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_PROBES);
    CHECK(kpm_check(3, 2, 7, false, 0, 0, 10, 0, 0.0, 4.0) == KPM_MU_LEN);
    CHECK(kpm_check(3, 2, 8, true, 10, 1, 10, 0, 0.0, 4.0) == KPM_LDZ);
    CHECK(kpm_check(3, 2, 8, false, 10, 1, 10, 0, 0.0, 4.0) == KPM_OK);   // hashed probes: ldz plays no part
    CHECK(kpm_check(3, 2, 8, true, 9, 2, 10, 0, 0.0, 4.0) == KPM_Z_ROWS);
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, 2, 0.0, 4.0) == KPM_AUTOMATIC);
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, -1, 0.0, 4.0) == KPM_AUTOMATIC);
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, 0, nan, 4.0) == KPM_NOT_FINITE);
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, 0, 0.0, inf) == KPM_NOT_FINITE);
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, 0, 4.0, 0.0) == KPM_EMPTY);
    CHECK(kpm_check(3, 2, 8, false, 0, 0, 10, 0, 1.0, 1.0) == KPM_EMPTY);
    for (int r = KPM_DEGREE; r <= KPM_EMPTY; ++r) CHECK(kpm_refusal_text((KpmRefusal)r)[0] != 0);
    CHECK(kpm_refusal_text(KPM_OK)[0] == 0);
    return 0;
}

static int sizes() {
    CHECK(kpm_steps(1) == 1 && kpm_steps(2) == 1 && kpm_steps(3) == 2 && kpm_steps(8) == 4 && kpm_steps(9) == 5 && kpm_steps(4096) == 2048);
    const KpmScalars<double> s = kpm_scalars<double>(-1.0, 3.0);
    CHECK(s.a1 == 0.5 && s.a2 == 1.0 && s.cT == 1.0);
    const KpmScalars<float> f = kpm_scalars<float>(0.0, 8.0);
    CHECK(f.a1 == 0.25f && f.a2 == 0.5f && f.cT == 4.0f);
    CHECK(kpm_tile_valid(0) && kpm_tile_valid(1) && kpm_tile_valid(2) && kpm_tile_valid(4) && kpm_tile_valid(8));
    CHECK(!kpm_tile_valid(3) && !kpm_tile_valid(16) && !kpm_tile_valid(-1));
    CHECK(kpm_tile_of(0, 1) == 1 && kpm_tile_of(0, 2) == 2 && kpm_tile_of(0, 3) == 4 && kpm_tile_of(0, 8) == 8 && kpm_tile_of(0, 9) == 8 &&
          kpm_tile_of(0, 256) == 8 && kpm_tile_of(2, 33) == 2);
    CHECK(kpm_padded(1, 1) == 1 && kpm_padded(3, 4) == 4 && kpm_padded(9, 8) == 16 && kpm_padded(33, 8) == 40 && kpm_padded(256, 8) == 256);
    // the products of a chunk fit the LDS budget, whatever the option says, and a chunk never drops below 256 entries
    for (int tile : {1, 2, 4, 8})
        for (size_t elem : {sizeof(float), sizeof(double)})
            for (unsigned opt : {0u, 256u, 512u, 1024u, 2048u, 4096u}) {
                const unsigned c = kpm_chunk_of(opt, tile, elem);
                CHECK(c >= 256 && (size_t)c * tile * elem <= kKpmProductBytes);
                CHECK(c <= (opt ? opt : 16 * 1024 / elem));
            }
    CHECK(kpm_chunk_of(0, 1, 8) == 2048 && kpm_chunk_of(0, 8, 8) == 512 && kpm_chunk_of(4096, 1, 4) == 4096 && kpm_chunk_of(256, 8, 8) == 256);
    CHECK(kpm_dot_elems(0) == 1 && kpm_dot_elems(1) == 1 && kpm_dot_elems(1024) == 1 && kpm_dot_elems(1025) == 3 &&
          kpm_dot_elems(1024ull * 1024) == 1025 && kpm_dot_elems(1024ull * 1024 + 1) == 1025 + 2 + 1);
    KpmLayout L;
    CHECK(kpm_layout(2049, 9, 8, 9, sizeof(double), &L));
    CHECK(L.kp == 16 && L.pe == 4);
    CHECK(L.block[0] == 0 && L.block[1] >= 2049 * 16 * 8 && L.block[2] - L.block[1] == L.block[1]);
    CHECK(L.part[0] >= L.block[2] + 2049 * 16 * 8 && L.part[1] - L.part[0] >= 4 * 16 * 8 && L.base >= L.part[2] + 4 * 16 * 8);
    CHECK(L.table >= L.base + 2 * 16 * 8 && L.total >= L.table + 10 * 9 * 8);
    for (size_t off : {L.block[1], L.block[2], L.part[0], L.part[1], L.part[2], L.base, L.table, L.total}) CHECK(off % 256 == 0);
    CHECK(!kpm_layout(~0ull / 8, 256, 8, 4096, sizeof(double), &L));   // does not fit: refused, nothing wraps
    CHECK(kpm_layout(1, 1, 1, 1, sizeof(float), &L) && L.total >= 3 * 4 + 3 * 4 + 8 + 16);
    return 0;
}

int main() {
    if (probes<double>() || probes<float>() || refusals() || sizes()) return 1;
    std::printf("kpm sanitize ok\n");
    return 0;
}

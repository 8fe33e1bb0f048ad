// Plain C++ restatement of the one-thread row sums of csr_spmv_blockwin (spalinalg_amd/csrc/spal_csr_blockwin.hip), for the CPU.
// A block of rows is taken in passes of `pass` entries counted from the block's first entry; a pass's products -- rounded once --
// lie in a strip in entry order; a row of at most 32 entries is summed left to right out of the strip, starting from `seed`
// where the row begins inside the pass and from the carry where the last pass's boundary cut it.  The kernel's seed is -0.0, the
// identity of IEEE addition: the first product is assigned, as in the reference (src/csr/ops/mul.rs:34).  With seed = +0.0, as
// the kernel first was, a row whose products are all -0.0 comes out +0.0.
// Rows of more than 32 entries are other lanes' business (tree sums): their y is left untouched.
#pragma once
#include <algorithm>
#include <cstdint>
#include <vector>

template <typename T>
void bw_thread_rows(const uint64_t *rowptr, const uint64_t *colind, const T *vals, const T *x, uint64_t r0, uint64_t r1,
                    uint64_t pass, T seed, T *y) {
    const uint64_t e0 = rowptr[r0], e1 = rowptr[r1];
    for (uint64_t i = r0; i < r1; ++i)   // empty rows: written apart, +0.0
        if (rowptr[i + 1] == rowptr[i]) y[i] = T(0);
    std::vector<T> strip[2] = {std::vector<T>(pass), std::vector<T>(pass)};
    T carry[2] = {T(0), T(0)};
    const uint64_t npass = (e1 - e0 + pass - 1) / pass;
    for (uint64_t p = 0; p < npass; ++p) {
        const uint64_t ps = e0 + p * pass, pe = std::min(ps + pass, e1), parity = p & 1u;
        for (uint64_t e = ps; e < pe; ++e) {
            volatile T prod = vals[e] * x[colind[e]];   // one rounding, kept apart from the addition
            strip[parity][e - ps] = prod;
        }
        for (uint64_t i = r0; i < r1; ++i) {
            const uint64_t rs = rowptr[i], re = rowptr[i + 1];
            const uint64_t a = std::max(rs, ps), b = std::min(re, pe);
            if (a >= b || re - rs > 32) continue;
            T acc = rs < ps ? carry[parity ^ 1u] : seed;
            for (uint64_t j = a - ps; j < b - ps; ++j) acc = acc + strip[parity][j];
            if (re <= pe) y[i] = acc;
            else carry[parity] = acc;
        }
    }
}

template <typename T>
void bw_thread_rows_blocks(uint64_t nrows, const uint64_t *rowptr, const uint64_t *colind, const T *vals, const T *x,
                           uint64_t block_rows, uint64_t pass, T seed, T *y) {
    for (uint64_t r0 = 0; r0 < nrows; r0 += block_rows)
        bw_thread_rows(rowptr, colind, vals, x, r0, std::min(r0 + block_rows, nrows), pass, seed, y);
}

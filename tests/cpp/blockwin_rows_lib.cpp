// C entry points of blockwin_rows.hpp, for tests/test_special_cases_host.py (ctypes): the block-window kernel's one-thread
// row sums on the CPU, against the oracle on the planted rows.  neg_zero_seed = 0 restates the sum as it was before the first
// product was assigned.
#include "blockwin_rows.hpp"

extern "C" {
void bw_thread_rows_f64(uint64_t nrows, const uint64_t *rowptr, const uint64_t *colind, const double *vals, const double *x,
                        uint64_t block_rows, uint64_t pass, int neg_zero_seed, double *y) {
    bw_thread_rows_blocks<double>(nrows, rowptr, colind, vals, x, block_rows, pass, neg_zero_seed ? -0.0 : 0.0, y);
}
void bw_thread_rows_f32(uint64_t nrows, const uint64_t *rowptr, const uint64_t *colind, const float *vals, const float *x,
                        uint64_t block_rows, uint64_t pass, int neg_zero_seed, float *y) {
    bw_thread_rows_blocks<float>(nrows, rowptr, colind, vals, x, block_rows, pass, neg_zero_seed ? -0.0f : 0.0f, y);
}
}

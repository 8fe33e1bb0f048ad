/* Plain C99 caller of the Krylov entry points of the C ABI (include/spal.h); needs a GPU.
 * A = tridiag(-1, 2, -1) of order 6 and b = A * (1, 2, 3, 4, 5, 6): CG converges in at most 6 steps, BiCGStab with the
 * ILU(0) factor (the exact LU of a tridiagonal matrix) leaves by the half-step exit after one; the host and the device
 * dot agree bit for bit. */
#include <math.h>
#include <stdio.h>
#include <string.h>

#include "spal.h"

#define CHECK(call)                                                                    \
    do {                                                                               \
        int st_ = (call);                                                              \
        if (st_ != SPAL_OK) {                                                          \
            fprintf(stderr, "%s failed: status %d: %s\n", #call, st_, spal_last_error()); \
            return 1;                                                                  \
        }                                                                              \
    } while (0)

int main(void) {
    const uint64_t rowptr[7] = {0, 2, 5, 8, 11, 14, 16};
    const uint64_t colind[16] = {0, 1, 0, 1, 2, 1, 2, 3, 2, 3, 4, 3, 4, 5, 4, 5};
    const double values[16] = {2, -1, -1, 2, -1, -1, 2, -1, -1, 2, -1, -1, 2, -1, -1, 2};
    const double want[6] = {1, 2, 3, 4, 5, 6}, b[6] = {0, 0, 0, 0, 0, 7};
    double x[6] = {0, 0, 0, 0, 0, 0}, d_host = 0, d_dev = 0;
    void *dv = NULL;
    spal_csr_t a = NULL, m = NULL;
    spal_krylov_info info;
    char plan[4096];
    int i;
    CHECK(spal_csr_create_f64(0, 6, 6, rowptr, 7, colind, 16, values, 16, &a));
    CHECK(spal_csr_krylov_f64(a, SPAL_KRYLOV_CG, NULL, b, 6, x, 6, 1e-12, 100, &info));
    if (info.reason != 0 || info.iterations < 1 || info.iterations > 6 || info.rhs_sq != 49.0) {
        fprintf(stderr, "cg: reason %d after %llu iterations\n", info.reason, (unsigned long long)info.iterations);
        return 1;
    }
    for (i = 0; i < 6; ++i)
        if (fabs(x[i] - want[i]) > 1e-9) { fprintf(stderr, "cg: x[%d] = %.17g\n", i, x[i]); return 1; }
    CHECK(spal_csr_ilu0(a, NULL, &m));
    memset(x, 0, sizeof x);
    CHECK(spal_csr_krylov_f64(a, SPAL_KRYLOV_BICGSTAB, m, b, 6, x, 6, 1e-12, 100, &info));
    if (info.reason != 0 || info.iterations != 1) {
        fprintf(stderr, "bicgstab: reason %d after %llu iterations\n", info.reason, (unsigned long long)info.iterations);
        return 1;
    }
    for (i = 0; i < 6; ++i)
        if (fabs(x[i] - want[i]) > 1e-12) { fprintf(stderr, "bicgstab: x[%d] = %.17g\n", i, x[i]); return 1; }
    if (spal_csr_krylov_f64(a, 2, NULL, b, 6, x, 6, 1e-12, 100, &info) != SPAL_ERR_INVALID_ARGUMENT ||
        !strstr(spal_last_error(), "method = 2")) { fprintf(stderr, "method 2 accepted\n"); return 1; }
    CHECK(spal_csr_describe(a, plan, sizeof plan));
    if (!strstr(plan, "\"krylov\": {\"method\": \"bicgstab\", \"preconditioned\": 1, \"iterations\": 1")) {
        fprintf(stderr, "describe: %s\n", plan);
        return 1;
    }
    /* the dot product: host definition and device kernel */
    CHECK(spal_dot_f64(values, values, 16, &d_host));
    CHECK(spal_dev_malloc(0, 17 * sizeof(double), &dv));
    CHECK(spal_memcpy_h2d(0, dv, values, sizeof values));
    CHECK(spal_dot_dev_f64(0, (const double *)dv, (const double *)dv, 16, (double *)dv + 16, NULL));
    CHECK(spal_device_synchronize(0));
    CHECK(spal_memcpy_d2h(0, &d_dev, (double *)dv + 16, sizeof d_dev));
    if (d_host != 34.0 || d_dev != d_host) { fprintf(stderr, "dot: host %g device %g\n", d_host, d_dev); return 1; }
    CHECK(spal_dev_free(0, dv));
    CHECK(spal_csr_destroy(m));
    CHECK(spal_csr_destroy(a));
    printf("krylov demo ok\n");
    return 0;
}

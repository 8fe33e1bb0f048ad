// ilu0_host.cpp -- the sequential ILU(0) loop of include/spal.h on one host core: what a caller without spal_*_ilu0 runs
// (tools/bench_ilu.py times it and compares its bits with the device's).  Build: g++ -O3 -ffp-contract=off.
//   ilu0_host <f64|f32> <n> <rowptr.u64> <colind.u64> <values.bin> <factor.bin>     prints the loop's milliseconds
#include <chrono>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <vector>

template <typename U>
static std::vector<U> read_all(const char *path, size_t count) {
    std::vector<U> v(count);
    FILE *f = fopen(path, "rb");
    if (!f || fread(v.data(), sizeof(U), count, f) != count) {
        fprintf(stderr, "cannot read %zu elements from %s\n", count, path);
        exit(2);
    }
    fclose(f);
    return v;
}

template <typename T>
static int run(uint64_t n, char **argv) {
    const std::vector<uint64_t> rp = read_all<uint64_t>(argv[3], n + 1);
    const uint64_t nnz = rp[n];
    const std::vector<uint64_t> ci = read_all<uint64_t>(argv[4], nnz);
    std::vector<T> f = read_all<T>(argv[5], nnz);
    std::vector<uint64_t> diag(n);
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t p = rp[i];
        while (p < rp[i + 1] && ci[p] < i) ++p;
        if (p == rp[i + 1] || ci[p] != i) {
            fprintf(stderr, "row %llu stores no diagonal entry\n", (unsigned long long)i);
            return 2;
        }
        diag[i] = p;
    }
    const auto t0 = std::chrono::steady_clock::now();
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t p1 = rp[i + 1];
        for (uint64_t p = rp[i]; p < diag[i]; ++p) {
            const uint64_t k = ci[p];
            const T w = f[p] / f[diag[k]];
            f[p] = w;
            uint64_t q = p + 1;
            for (uint64_t pu = diag[k] + 1; pu < rp[k + 1] && q < p1; ++pu) {
                const uint64_t j = ci[pu];
                while (q < p1 && ci[q] < j) ++q;
                if (q < p1 && ci[q] == j) {
                    f[q] = f[q] - w * f[pu];
                    ++q;
                }
            }
        }
    }
    const double ms = std::chrono::duration<double, std::milli>(std::chrono::steady_clock::now() - t0).count();
    FILE *out = fopen(argv[6], "wb");
    if (!out || fwrite(f.data(), sizeof(T), nnz, out) != nnz) {
        fprintf(stderr, "cannot write %s\n", argv[6]);
        return 2;
    }
    fclose(out);
    printf("%.3f\n", ms);
    return 0;
}

int main(int argc, char **argv) {
    if (argc != 7) {
        fprintf(stderr, "usage: ilu0_host <f64|f32> <n> <rowptr.u64> <colind.u64> <values.bin> <factor.bin>\n");
        return 2;
    }
    const uint64_t n = strtoull(argv[2], nullptr, 10);
    return strcmp(argv[1], "f32") ? run<double>(n, argv) : run<float>(n, argv);
}

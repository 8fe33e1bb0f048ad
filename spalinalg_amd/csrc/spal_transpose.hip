// spal_transpose.hip -- CSR <-> CSC on the device: a stable radix sort (spal_coo_sort.hip) of the entries by their
// minor index.
#include "coo_internal.hpp"

namespace spal {

// --------------------------------------------------------------------------
// compressed-by-major -> compressed-by-minor (CSR <-> CSC, transpose)
// Device twin of the counting sort of src/csr.rs:358-406 /
// src/csr/conv/csc.rs:4-52 / src/csc/conv/csr.rs:4-52: a stable sort of the
// entries by their minor index keeps the major indices ascending inside every
// minor slice, so the result is exactly the reference's (same order, same
// values -- entries are only moved).
// --------------------------------------------------------------------------
// major index of every entry (one thread per major slice; slices are short)
__global__ __launch_bounds__(256) void expand_major(const uint32_t *__restrict__ ptr, uint32_t nmajor,
                                                    uint32_t *__restrict__ major) {
    const uint64_t m = (uint64_t)blockIdx.x * 256 + threadIdx.x;
    if (m >= nmajor) return;
    for (uint32_t p = ptr[m]; p < ptr[m + 1]; ++p) major[p] = (uint32_t)m;
}

template <typename T>
static int transpose_t(uint64_t nmajor, uint64_t nminor, uint64_t nnz, const uint32_t *d_ptr, const uint32_t *d_ind,
                       const T *d_val, hipStream_t st, OpArrays &out) {
    DevBuf work, major;   // (scratch, freed on return -- behind the synchronise below)
    SPAL_TRY(out.alloc(nminor, nnz, sizeof(T), st));
    if (nnz == 0) {
        SPAL_HIP_TRY(hipMemsetAsync(out.ptr, 0, (nminor + 1) * 4, st));
    } else {
        const CooWorkspace ws = coo_workspace_layout(nnz, nminor, sizeof(T));
        SPAL_HIP_TRY(work.alloc(ws.bytes));
        SPAL_HIP_TRY(major.alloc(nnz * 4));
        SortBuffers<T> sb = coo_workspace_sort_buffers<T>((char *)work.p, ws);
        hipLaunchKernelGGL(expand_major, dim3((uint32_t)((nmajor + 255) / 256)), dim3(256), 0, st, d_ptr,
                           (uint32_t)nmajor, major.as<uint32_t>());
        int cur = 0;
        SPAL_HIP_TRY(radix_sort_bits<T>(sb, nnz, 0, bits_for(nminor), cur, st, d_ind,
                                        major.as<uint32_t>(), d_val));
        launch_row_starts(sb.key[cur], (uint32_t)nnz, (uint32_t)nminor, out.ptr, st);
        SPAL_HIP_TRY(hipMemcpyAsync(out.ind, sb.aux[cur], nnz * 4, hipMemcpyDeviceToDevice, st));
        SPAL_HIP_TRY(hipMemcpyAsync(out.val, sb.val[cur], nnz * sizeof(T), hipMemcpyDeviceToDevice, st));
        SPAL_HIP_TRY(hipGetLastError());
    }
    SPAL_HIP_TRY(hipStreamSynchronize(st));
    return SPAL_OK;
}

int transpose_device(int device, int elem_size, uint64_t nmajor, uint64_t nminor, uint64_t nnz, const uint32_t *d_ptr,
                     const uint32_t *d_ind, const void *d_val, hipStream_t st, OpArrays &out) {
    return elem_size == 8 ? transpose_t<double>(nmajor, nminor, nnz, d_ptr, d_ind, (const double *)d_val, st, out)
                          : transpose_t<float>(nmajor, nminor, nnz, d_ptr, d_ind, (const float *)d_val, st, out);
}

}  // namespace spal

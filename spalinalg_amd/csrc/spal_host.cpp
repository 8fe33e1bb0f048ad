// spal_host.cpp -- host-only parts of libspal_hip.so: error state, the
// constructor invariants of the reference, the row partitioner, the level analysis of the triangular solve and the
// epilogue of describe()'s per-operation objects.  Nothing here touches a device.
#include "spal_internal.hpp"

namespace spal {

std::string &last_error_ref() {
    static thread_local std::string msg;
    return msg;
}

int fail(int status, const char *fmt, ...) {
    char buf[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    last_error_ref() = buf;
    return status;
}

unsigned host_threads() {
    static unsigned n = [] {
        unsigned h = std::thread::hardware_concurrency();
        if (const char *e = getenv("SPAL_HOST_THREADS")) {
            int v = atoi(e);
            if (v > 0) return (unsigned)v;
        }
        if (h == 0) h = 1;
        return std::min(h, 32u);
    }();
    return n;
}

void parallel_for(uint64_t n, const std::function<void(uint64_t, uint64_t, unsigned)> &fn,
                  uint64_t min_chunk) {
    if (n == 0) return;
    unsigned nt = host_threads();
    uint64_t max_by_size = (n + min_chunk - 1) / min_chunk;
    if (max_by_size < nt) nt = (unsigned)max_by_size;
    if (nt <= 1) {
        fn(0, n, 0);
        return;
    }
    std::vector<std::thread> th;
    th.reserve(nt);
    uint64_t per = (n + nt - 1) / nt;
    for (unsigned t = 0; t < nt; ++t) {
        uint64_t b = std::min<uint64_t>(n, (uint64_t)t * per);
        uint64_t e = std::min<uint64_t>(n, b + per);
        if (b >= e) break;
        th.emplace_back([&fn, b, e, t] { fn(b, e, t); });
    }
    for (auto &t : th) t.join();
}

// ---------------------------------------------------------------------------
// CsrMatrix::new / CscMatrix::new  (reference src/csr.rs:144-156,
// src/csc.rs:144-156).  The reference asserts in sequence, each assertion over
// the whole array, so "the first assertion that fails" is the lowest ordinal
// that fails anywhere -- which lets the three O(nnz) scans run in parallel.
// ---------------------------------------------------------------------------
int compressed_validate(uint64_t nrows, uint64_t ncols, bool major_is_rows,
                        const uint64_t *ptr, uint64_t ptr_len, const uint64_t *ind,
                        uint64_t ind_len, uint64_t val_len) {
    const uint64_t nmajor = major_is_rows ? nrows : ncols;
    const uint64_t nminor = major_is_rows ? ncols : nrows;
    if (!(nrows > 0)) return 1;
    if (!(ncols > 0)) return 2;
    if (!(ptr_len == nmajor + 1)) return 3;
    if (!(ptr[0] == 0)) return 4;
    if (!(ind_len == ptr[nmajor])) return 5;
    if (!(val_len == ptr[nmajor])) return 6;
    const unsigned nt = host_threads();
    std::vector<int> bad7(nt, 0), bad8(nt, 0), bad9(nt, 0);
    parallel_for(nmajor, [&](uint64_t b, uint64_t e, unsigned t) {
        for (uint64_t i = b; i < e; ++i)
            if (!(ptr[i] <= ptr[i + 1])) { bad7[t] = 1; break; }
    });
    for (int f : bad7) if (f) return 7;
    parallel_for(ind_len, [&](uint64_t b, uint64_t e, unsigned t) {
        for (uint64_t p = b; p < e; ++p)
            if (!(ind[p] < nminor)) { bad8[t] = 1; break; }
    });
    for (int f : bad8) if (f) return 8;
    // ptr is now known monotone with ptr[nmajor] == ind_len: slices are in range
    parallel_for(nmajor, [&](uint64_t b, uint64_t e, unsigned t) {
        for (uint64_t m = b; m < e && !bad9[t]; ++m)
            for (uint64_t p = ptr[m]; p + 1 < ptr[m + 1]; ++p)
                if (!(ind[p] < ind[p + 1])) { bad9[t] = 1; break; }
    });
    for (int f : bad9) if (f) return 9;
    return 0;
}

// The epilogue of every object a sparse operation adds to a describe() line (spal_ops.hpp): `, "<key>": <body>` goes
// where the line's closing brace was, and the brace behind it.
int describe_append(char *buf, size_t buf_len, const char *key, const std::string &body) {
    if (body.empty()) return SPAL_OK;
    const size_t len = strnlen(buf, buf_len), add = strlen(key) + body.size() + 6;   // `, "` and `": ` around the key
    if (len == 0 || buf[len - 1] != '}' || len + add + 1 > buf_len)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "describe: buffer of %zu bytes too small", buf_len);
    snprintf(buf + len - 1, buf_len - (len - 1), ", \"%s\": %s}", key, body.c_str());
    return SPAL_OK;
}

const char *invariant_text(int reason, bool csr) {
    switch (reason) {
        case 1: return "nrows > 0";
        case 2: return "ncols > 0";
        case 3: return csr ? "rowptr.len() == nrows + 1" : "colptr.len() == ncols + 1";
        case 4: return csr ? "rowptr[0] == 0" : "colptr[0] == 0";
        case 5: return csr ? "colind.len() == rowptr[nrows]" : "rowind.len() == colptr[ncols]";
        case 6: return csr ? "values.len() == rowptr[nrows]" : "values.len() == colptr[ncols]";
        case 7: return csr ? "rowptr is sorted" : "colptr is sorted";
        case 8: return csr ? "every colind < ncols" : "every rowind < nrows";
        case 9: return csr ? "colind strictly increasing inside each row"
                           : "rowind strictly increasing inside each column";
        default: return "ok";
    }
}

// ---------------------------------------------------------------------------
// Level analysis of the triangular solve.  level_of[i] = 0 when row i uses no off-diagonal entry of the
// chosen triangle, else 1 + the largest level of the rows it reads.  One sequential pass, ascending rows for the lower
// triangle and descending for the upper one, so every level read is final.  dpos (optional) receives, per row, the
// position of its first entry with column >= row: the strictly lower entries end there, the diagonal (if stored) sits
// there, the strictly upper ones follow it.
// ---------------------------------------------------------------------------
template <typename Idx, typename Lev>
int trsv_levels_impl(uint64_t n, const Idx *rowptr, const Idx *colind, int uplo, Lev *level_of, uint64_t *nlevels,
                     uint64_t *first_missing_diag, Idx *dpos) {
    uint64_t top = 0, missing = n;
    for (uint64_t k = 0; k < n; ++k) {
        const uint64_t i = uplo ? n - 1 - k : k;
        const uint64_t b = rowptr[i], e = rowptr[i + 1];
        if (e > b && (uint64_t)colind[e - 1] >= n)   // columns ascend: the last one is the largest
            return fail(SPAL_ERR_INVALID_ARGUMENT,
                        "triangular solve: the matrix is not square (row %llu stores column %llu, n = %llu)",
                        (unsigned long long)i, (unsigned long long)colind[e - 1], (unsigned long long)n);
        uint64_t p = b, lev = 0;
        if (!uplo) {
            for (; p < e && (uint64_t)colind[p] < i; ++p) lev = std::max<uint64_t>(lev, (uint64_t)level_of[colind[p]] + 1);
        } else {
            // (a binary search would not change the O(nnz) bound: the entries skipped here are read once)
            while (p < e && (uint64_t)colind[p] < i) ++p;
        }
        const bool has_diag = p < e && (uint64_t)colind[p] == i;
        if (dpos) dpos[i] = (Idx)p;
        if (!has_diag && (missing == n || uplo)) missing = i;   // descending walk: the last one met is the first row
        if (uplo)
            for (uint64_t q = p + (has_diag ? 1 : 0); q < e; ++q)
                lev = std::max<uint64_t>(lev, (uint64_t)level_of[colind[q]] + 1);
        level_of[i] = (Lev)lev;
        top = std::max(top, lev);
    }
    *nlevels = n ? top + 1 : 0;
    *first_missing_diag = missing;
    return SPAL_OK;
}

int trsv_levels_u32(uint64_t n, const uint32_t *rowptr, const uint32_t *colind, int uplo, uint32_t *level_of,
                    uint64_t *nlevels, uint64_t *first_missing_diag, uint32_t *dpos) {
    return trsv_levels_impl<uint32_t, uint32_t>(n, rowptr, colind, uplo, level_of, nlevels, first_missing_diag, dpos);
}

int trsv_missing_diag(const char *fn, uint64_t row) {
    return fail(SPAL_ERR_INVALID_ARGUMENT,
                "%s: row %llu stores no diagonal entry (a non-unit triangular solve divides by it)", fn,
                (unsigned long long)row);
}

// ---------------------------------------------------------------------------
// Multicolour ordering: what spal_colour_greedy checks of its arrays before it reads through them.
// ---------------------------------------------------------------------------
static int colour_check_pattern(const char *fn, uint64_t n, const uint64_t *rowptr, const uint64_t *colind) {
    if (rowptr[0] != 0) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: rowptr[0] = %llu, not 0", fn, (unsigned long long)rowptr[0]);
    for (uint64_t i = 0; i < n; ++i)
        if (rowptr[i] > rowptr[i + 1])
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: rowptr is not sorted (rowptr[%llu] > rowptr[%llu])", fn,
                        (unsigned long long)i, (unsigned long long)(i + 1));
    if (!colind && rowptr[n]) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null array", fn);
    for (uint64_t p = 0; p < rowptr[n]; ++p)
        if (colind[p] >= n)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: the matrix is not square (entry %llu stores column %llu, n = %llu)", fn,
                        (unsigned long long)p, (unsigned long long)colind[p], (unsigned long long)n);
    return SPAL_OK;
}

}  // namespace spal

using namespace spal;

extern "C" {

const char *spal_last_error(void) { return last_error_ref().c_str(); }

const char *spal_version(void) { return "spalinalg_amd 0.1.0 (gfx950)"; }

int spal_csr_validate(uint64_t nrows, uint64_t ncols, const uint64_t *rowptr,
                      uint64_t rowptr_len, const uint64_t *colind, uint64_t colind_len,
                      uint64_t values_len, int *reason) {
    if (reason) *reason = 0;
    if ((!rowptr && rowptr_len) || (!colind && colind_len))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csr_validate: null array");
    int r = compressed_validate(nrows, ncols, true, rowptr, rowptr_len, colind, colind_len,
                                values_len);
    if (reason) *reason = r;
    if (r) return fail(SPAL_ERR_INVARIANT, "CsrMatrix::new would panic: assertion failed: %s",
                       invariant_text(r, true));
    return SPAL_OK;
}

int spal_csc_validate(uint64_t nrows, uint64_t ncols, const uint64_t *colptr,
                      uint64_t colptr_len, const uint64_t *rowind, uint64_t rowind_len,
                      uint64_t values_len, int *reason) {
    if (reason) *reason = 0;
    if ((!colptr && colptr_len) || (!rowind && rowind_len))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_csc_validate: null array");
    int r = compressed_validate(nrows, ncols, false, colptr, colptr_len, rowind, rowind_len,
                                values_len);
    if (reason) *reason = r;
    if (r) return fail(SPAL_ERR_INVARIANT, "CscMatrix::new would panic: assertion failed: %s",
                       invariant_text(r, false));
    return SPAL_OK;
}

int spal_partition_rows(const uint64_t *rowptr, uint64_t nrows, uint32_t nparts,
                        uint64_t *bounds) {
    if (!rowptr || !bounds || nparts == 0)
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_partition_rows: null array or nparts == 0");
    const uint64_t nnz = rowptr[nrows];
    bounds[0] = 0;
    for (uint32_t g = 1; g < nparts; ++g) {
        // first row whose starting offset reaches g/nparts of the entries;
        // rows (not entries) are split evenly when the matrix is empty
        uint64_t cut;
        if (nnz == 0) {
            cut = (uint64_t)(((unsigned __int128)nrows * g) / nparts);
        } else {
            const uint64_t target = (uint64_t)(((unsigned __int128)nnz * g) / nparts);
            cut = (uint64_t)(std::lower_bound(rowptr, rowptr + nrows + 1, target) - rowptr);
            if (cut > nrows) cut = nrows;
        }
        bounds[g] = std::max(cut, bounds[g - 1]);
    }
    bounds[nparts] = nrows;
    return SPAL_OK;
}

int spal_trsv_levels(uint64_t n, const uint64_t *rowptr, const uint64_t *colind, int uplo, int unit_diag,
                     uint64_t *level_of, uint64_t *nlevels) {
    if (!rowptr || !level_of || !nlevels || (!colind && n && rowptr[n]))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_trsv_levels: null array");
    if ((uplo != 0 && uplo != 1) || (unit_diag != 0 && unit_diag != 1))
        return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_trsv_levels: uplo must be 0 (lower) or 1 (upper) and unit_diag 0 or 1");
    uint64_t missing = n;
    SPAL_TRY((trsv_levels_impl<uint64_t, uint64_t>(n, rowptr, colind, uplo, level_of, nlevels, &missing, nullptr)));
    if (!unit_diag && missing < n) return trsv_missing_diag("spal_trsv_levels", missing);
    return SPAL_OK;
}

// The text of include/spal.h as it reads: vertices by descending key, the smallest colour no visited neighbour has.
int spal_colour_greedy(uint64_t n, const uint64_t *rowptr, const uint64_t *colind, uint64_t seed, uint64_t *colour,
                       uint64_t *ncolours) {
    const char *fn = "spal_colour_greedy";
    if (!rowptr || !ncolours || (!colour && n)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null array", fn);
    SPAL_TRY(colour_check_pattern(fn, n, rowptr, colind));
    const uint64_t nnz = rowptr[n];
    // the rows of A^T: a counting sort of the entries by column
    std::vector<uint64_t> tptr(n + 1, 0), tind(nnz);
    for (uint64_t p = 0; p < nnz; ++p) ++tptr[colind[p] + 1];
    for (uint64_t j = 0; j < n; ++j) tptr[j + 1] += tptr[j];
    {
        std::vector<uint64_t> next(tptr.begin(), tptr.end() - 1);
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) tind[next[colind[p]]++] = i;
    }
    std::vector<std::pair<uint32_t, uint64_t>> order(n);   // (key, vertex); keys are distinct
    for (uint64_t i = 0; i < n; ++i) order[i] = {colour_mix32((uint32_t)(i + seed)), i};
    std::sort(order.begin(), order.end(), [](const auto &a, const auto &b) { return a.first > b.first; });
    const uint64_t none = ~0ull;
    std::fill(colour, colour + n, none);
    std::vector<uint64_t> taken(n, none);   // taken[c] == v: a visited neighbour of v has colour c
    uint64_t top = 0;
    for (const auto &kv : order) {
        const uint64_t v = kv.second;
        for (uint64_t p = rowptr[v]; p < rowptr[v + 1]; ++p)
            if (colind[p] != v && colour[colind[p]] != none) taken[colour[colind[p]]] = v;
        for (uint64_t p = tptr[v]; p < tptr[v + 1]; ++p)
            if (tind[p] != v && colour[tind[p]] != none) taken[colour[tind[p]]] = v;
        uint64_t c = 0;
        while (taken[c] == v) ++c;   // at most deg(v) colours are taken and deg(v) < n: c < n
        colour[v] = c;
        top = std::max(top, c + 1);
    }
    *ncolours = top;
    return SPAL_OK;
}

int spal_amg_default_params(spal_amg_params *params) {
    if (!params) return fail(SPAL_ERR_INVALID_ARGUMENT, "spal_amg_default_params: null argument");
    *params = spal_amg_params{0, 16, 64, 2, 16, 1, 2.0 / 3.0, 1.0};
    return SPAL_OK;
}

// The aggregation text of include/spal.h as it reads: degrees, vertices by descending priority, roots,
// the join, the numbering.
int spal_amg_aggregate(uint64_t n, const uint64_t *rowptr, const uint64_t *colind, uint64_t seed, uint64_t *agg,
                       uint64_t *nagg) {
    const char *fn = "spal_amg_aggregate";
    if (!rowptr || !nagg || (!agg && n)) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null array", fn);
    SPAL_TRY(colour_check_pattern(fn, n, rowptr, colind));
    const uint64_t nnz = rowptr[n];
    // the rows of A^T: a counting sort of the entries by column (rows ascending inside a column)
    std::vector<uint64_t> tptr(n + 1, 0), tind(nnz);
    for (uint64_t p = 0; p < nnz; ++p) ++tptr[colind[p] + 1];
    for (uint64_t j = 0; j < n; ++j) tptr[j + 1] += tptr[j];
    {
        std::vector<uint64_t> next(tptr.begin(), tptr.end() - 1);
        for (uint64_t i = 0; i < n; ++i)
            for (uint64_t p = rowptr[i]; p < rowptr[i + 1]; ++p) tind[next[colind[p]]++] = i;
    }
    // the neighbours of every vertex, each once (the rows of a pattern need not be in order here)
    std::vector<uint64_t> nptr(n + 1, 0), nbr;
    nbr.reserve(2 * nnz);
    std::vector<uint64_t> row;
    for (uint64_t i = 0; i < n; ++i) {
        row.assign(colind + rowptr[i], colind + rowptr[i + 1]);
        row.insert(row.end(), tind.begin() + tptr[i], tind.begin() + tptr[i + 1]);
        std::sort(row.begin(), row.end());
        row.erase(std::unique(row.begin(), row.end()), row.end());
        for (uint64_t j : row)
            if (j != i) nbr.push_back(j);
        nptr[i + 1] = nbr.size();
    }
    std::vector<uint64_t> prio(n);
    for (uint64_t i = 0; i < n; ++i) {
        const uint64_t deg = std::min<uint64_t>(nptr[i + 1] - nptr[i], 0x7fffffffull);
        prio[i] = deg << 32 | colour_mix32((uint32_t)(i + seed));
    }
    std::vector<uint64_t> order(n);
    for (uint64_t i = 0; i < n; ++i) order[i] = i;
    std::sort(order.begin(), order.end(), [&](uint64_t a, uint64_t b) { return prio[a] > prio[b]; });
    std::vector<char> root(n, 0);
    for (const uint64_t v : order) {
        bool free = true;
        for (uint64_t p = nptr[v]; p < nptr[v + 1] && free; ++p) free = !root[nbr[p]];
        root[v] = free ? 1 : 0;
    }
    std::vector<uint64_t> number(n, 0);
    uint64_t count = 0;
    for (uint64_t i = 0; i < n; ++i)
        if (root[i]) number[i] = count++;
    for (uint64_t i = 0; i < n; ++i) {
        uint64_t r = i;
        if (!root[i]) {
            bool any = false;
            for (uint64_t p = nptr[i]; p < nptr[i + 1]; ++p) {
                const uint64_t j = nbr[p];
                if (root[j] && (!any || prio[j] > prio[r])) {
                    r = j;
                    any = true;
                }
            }
        }
        agg[i] = number[r];
    }
    *nagg = count;
    return SPAL_OK;
}

int spal_perm_from_colours(uint64_t n, const uint64_t *colour, uint64_t *perm) {
    const char *fn = "spal_perm_from_colours";
    if ((!colour || !perm) && n) return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: null array", fn);
    std::vector<uint64_t> start(n + 1, 0);
    for (uint64_t i = 0; i < n; ++i) {
        if (colour[i] >= n)
            return fail(SPAL_ERR_INVALID_ARGUMENT, "%s: colour[%llu] = %llu is not below n = %llu", fn, (unsigned long long)i,
                        (unsigned long long)colour[i], (unsigned long long)n);
        ++start[colour[i] + 1];
    }
    for (uint64_t c = 0; c < n; ++c) start[c + 1] += start[c];
    for (uint64_t i = 0; i < n; ++i) perm[start[colour[i]]++] = i;   // rows ascending inside a colour: stable
    return SPAL_OK;
}

}  // extern "C"

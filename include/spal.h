/*
 * spal.h -- C ABI of libspal_hip.so: the MI355X (gfx950) SpMV / assembly path
 * that sits underneath spalinalg's public CsrMatrix / CscMatrix / CooMatrix
 * types (reference: lokyhark/spalinalg, paths below relative to its root).
 *
 * The reference has no FFI of its own; every entry point here
 * names the reference interface it would be bound under.  The Rust-side
 * binding a maintainer adds is shown in INTEGRATION.md and rust_shim/.
 *
 * Conventions
 *  - plain C: pointers + sizes only, no C++ types, no exceptions, no torch.
 *  - `usize` of the reference == uint64_t here (x86-64 Linux).
 *  - host arrays are BORROWED for the duration of the call; device copies are
 *    owned by the opaque handle and released by *_destroy.
 *  - every function returns a spal_status; on failure a thread-local message
 *    is available from spal_last_error().  The reference's convention is to
 *    panic on a contract violation (assert!, src/csr.rs:144-156); a binding
 *    turns any non-zero status into panic!() to keep that behaviour.
 *  - scalars: exactly the two `Scalar` impls, f32 and f64 (src/scalar.rs:56-57).
 *  - there is NO CPU fallback: without a usable HIP device every compute
 *    entry point fails with SPAL_ERR_NO_DEVICE / SPAL_ERR_HIP.
 */
#ifndef SPAL_H
#define SPAL_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef enum spal_status {
    SPAL_OK = 0,
    SPAL_ERR_INVALID_ARGUMENT = 1, /* null pointer, x.len() != ncols (src/csr/ops/mul.rs:9) ... */
    SPAL_ERR_INVARIANT = 2,        /* the reference constructor would panic (src/csr.rs:144-156) */
    SPAL_ERR_HIP = 3,              /* a HIP runtime call failed */
    SPAL_ERR_OUT_OF_MEMORY = 4,
    SPAL_ERR_UNSUPPORTED = 5,      /* shape does not fit the device's 32-bit index format */
    SPAL_ERR_NO_DEVICE = 6,
    SPAL_ERR_INDEX_OUT_OF_BOUNDS = 7 /* COO entry outside the matrix (src/coo.rs:432-433) */
} spal_status;

/* Opaque device-resident matrices. */
typedef struct spal_csr *spal_csr_t; /* mirrors CsrMatrix<T>, src/csr.rs:66-72 */
typedef struct spal_csc *spal_csc_t; /* mirrors CscMatrix<T>, src/csc.rs:66-72 */
typedef struct spal_coo *spal_coo_t; /* mirrors CooMatrix<T>, src/coo.rs:53-57 (SoA on device) */
typedef struct spal_mg *spal_mg_t;          /* the GPUs of one node + their RCCL communicators */
typedef struct spal_mg_csr *spal_mg_csr_t;  /* a CsrMatrix partitioned by rows over them */
typedef struct spal_amg *spal_amg_t;        /* an aggregation multigrid hierarchy (below) */
typedef struct spal_fsai *spal_fsai_t;      /* a factorised sparse approximate inverse (below) */

/* ---- library ---------------------------------------------------------- */
const char *spal_last_error(void);   /* thread-local, never NULL */
const char *spal_version(void);
int spal_device_count(int *count);   /* 0 devices is SPAL_OK with *count = 0 */

/* ---- host-side checks (no device needed) ------------------------------- */
/* The assertions of CsrMatrix::new (src/csr.rs:144-156), in order.  On
 * SPAL_ERR_INVARIANT *reason (may be NULL) receives the 1-based ordinal of
 * the first assertion that fails:  1 nrows>0, 2 ncols>0, 3 rowptr.len()==
 * nrows+1, 4 rowptr[0]==0, 5 colind.len()==rowptr[nrows], 6 values.len()==
 * rowptr[nrows], 7 rowptr sorted, 8 colind in range, 9 colind strictly
 * increasing inside each row. */
int spal_csr_validate(uint64_t nrows, uint64_t ncols,
                      const uint64_t *rowptr, uint64_t rowptr_len,
                      const uint64_t *colind, uint64_t colind_len,
                      uint64_t values_len, int *reason);
/* CscMatrix::new (src/csc.rs:144-156): same ordinals with colptr / rowind. */
int spal_csc_validate(uint64_t nrows, uint64_t ncols,
                      const uint64_t *colptr, uint64_t colptr_len,
                      const uint64_t *rowind, uint64_t rowind_len,
                      uint64_t values_len, int *reason);
/* Contiguous row ranges with balanced stored entries, for the row-partitioned
 * multi-GPU product.  bounds has nparts+1 entries,
 * bounds[0] = 0, bounds[nparts] = nrows, non-decreasing. */
int spal_partition_rows(const uint64_t *rowptr, uint64_t nrows,
                        uint32_t nparts, uint64_t *bounds);

/* ---- CSR: y = A * x ------------------------------------------------------
 * Replaces the reference's only route to A*x, `&a * &x_as_matrix`
 * (`impl Mul for &CsrMatrix<T>`, src/csr/ops/mul.rs:5-59); bound as
 * `impl Mul<&[T]> for &CsrMatrix<T>`.
 * create: borrows rowptr()/colind()/values() (src/csr.rs:228-258), checks
 * the constructor's invariants, narrows indices to 32 bits and uploads.
 * Limits: nrows, ncols < 2^32.  The number of stored entries is not limited
 * (the reference's offsets are usize, src/csr.rs:66-72): beyond 2^32 - 65537
 * entries the handle keeps the matrix as row blocks with 32-bit offsets each
 * (spal_csr_describe reports "kernel": "row_blocks" and the cuts); products,
 * download, options and autotune work on the whole; spal_csr_to_csc is then
 * refused (SPAL_ERR_UNSUPPORTED), and so are CSC / COO handles of that size. */
int spal_csr_create_f64(int device, uint64_t nrows, uint64_t ncols,
                        const uint64_t *rowptr, uint64_t rowptr_len,
                        const uint64_t *colind, uint64_t colind_len,
                        const double *values, uint64_t values_len,
                        spal_csr_t *out);
int spal_csr_create_f32(int device, uint64_t nrows, uint64_t ncols,
                        const uint64_t *rowptr, uint64_t rowptr_len,
                        const uint64_t *colind, uint64_t colind_len,
                        const float *values, uint64_t values_len,
                        spal_csr_t *out);
int spal_csr_destroy(spal_csr_t a);
/* nrows()/ncols()/nnz() (src/csr.rs:200-222, :287-289); elem_size 4 or 8. */
int spal_csr_shape(spal_csr_t a, uint64_t *nrows, uint64_t *ncols,
                   uint64_t *nnz, int *elem_size);
/* What a product returns (CSR and CSC, SpMV and SpMM; DESIGN 3.2d has the table per path).
 * NaN and +-inf -- in x or stored in the matrix -- reach exactly the rows that reference them, on every path; a stored
 * zero is an entry like any other (0 * inf is the reference's NaN); the sign and payload of a NaN are not promised.
 * The paths that keep the reference's order of additions -- the stream, sliding-window, column-panel and column-blocked
 * kernels, the block-window kernel's rows of at most 32 entries, the short part of the row split where its plan streams
 * it, CSC handles on their default route, SpMM, the row shards -- return the reference's BITS: the first product of a
 * row is assigned (src/csr/ops/mul.rs:34), so a row whose products are all -0.0 gives -0.0; subnormals are not flushed;
 * rows without stored entries give +0.0.  The tree-summed and atomic paths -- vector kernel, overflow kernel, listed
 * rows of the row split, the block-window kernel's longer rows, the CSC scatter routes ("kernel" = 1) -- agree with
 * the reference to 1e-10 (f64) / 1e-4 (f32), normwise and against sum |a||x|; they accumulate from +0.0 and may return
 * +0.0 where the reference returns -0.0; they keep subnormals too (the f32 atomic adds do not flush them on gfx950). */
/* Host convenience: H2D x, kernel, D2H y.  x_len must equal ncols and y_len
 * nrows (mirrors assert_eq! at src/csr/ops/mul.rs:9).  y is fully
 * overwritten; rows without stored entries give 0.0. */
int spal_csr_spmv_f64(spal_csr_t a, const double *x, uint64_t x_len,
                      double *y, uint64_t y_len);
int spal_csr_spmv_f32(spal_csr_t a, const float *x, uint64_t x_len,
                      float *y, uint64_t y_len);
/* Timed path: x (ncols) and y (nrows) are DEVICE pointers on the handle's
 * device; the launch is enqueued on `stream` (a hipStream_t, NULL = the
 * default stream) and not synchronised.  Safe to call concurrently on one
 * handle (read-only). */
int spal_csr_spmv_dev_f64(spal_csr_t a, const double *x_dev, double *y_dev,
                          void *stream);
int spal_csr_spmv_dev_f32(spal_csr_t a, const float *x_dev, float *y_dev,
                          void *stream);
/* Copies the device matrix back into caller arrays shaped like the
 * reference's fields (rowptr nrows+1, colind nnz, values nnz). */
int spal_csr_download_f64(spal_csr_t a, uint64_t *rowptr, uint64_t *colind,
                          double *values);
int spal_csr_download_f32(spal_csr_t a, uint64_t *rowptr, uint64_t *colind,
                          float *values);
/* Kernel plan knobs (tuning / tests).  Keys: "kernel" (0 = auto, 1 = vector,
 * 2 = stream), "rows_per_block", "lanes_per_row", "lds_x" (-1 auto/0/1),
 * "unroll", "threads", "col16" (long rows: 16-bit columns, default 1) (vector
 * kernel); "rows_per_tile" (0 auto, 256, 128, 64, 32, 24, 16, 12, 8),
 * "tiles_per_wave", "persistent", "persistent_blocks" (0 = what the device
 * holds at once), "nt_store", "stream_global", "window_pages" (0 auto; LDS x
 * window budget in 256-column pages), "stream_row_max" (64-row tiles with a
 * longer row go to the overflow kernel; default 128), "skew" (-1 auto, 0, 1:
 * skewed LDS product strips), "slide" (-1 auto / 0: the sliding-window kernel
 * and its ring-addressed x window for band-like plans), "slide_on" (0 / 1:
 * launch it), "rowrec" (-1 auto / 0 / 1: rows of one even length in [12, 16]
 * under the sliding kernel stream one 20- or 24-byte record per row instead of
 * the row's 16-bit columns), "rowrec_on" (0 / 1: launch that form),
 * "valpack" (-1 auto / 0 / 1: an f64 handle with row records whose values are
 * all k * 2^e for one e, k inside 53 bits for rows of 12 and 54 bits for rows of
 * 14 or 16 entries, no NaN, Inf or -0.0, streams one fixed-point block of 80 /
 * 96 / 112 bytes per row instead of the row's values; the values stay resident
 * beside the blocks), "valpack_on" (0 / 1: launch that form),
 * "uniform_rows" (0 / 1: super-tiles whose rows all have one length
 * do not read rowptr), "prefetch" (1 / 2 tiles of loads ahead), "place_tries"
 * (autotune), "split_tiles" (1 default / 0: the sliding kernel computes tiles
 * above 1024 entries whose halves fit in two passes instead of leaving them to
 * the overflow kernel), "xcd_chunk", "walk_blocks" (stream kernel); "cblock"
 * (-1 auto / 0 / 1: the column-blocked kernels for columns anywhere),
 * "cblock_form" (-1 by the entries a row holds per column block / 0 entry-
 * parallel / 1 rows form), "cblock_rows", "cblock_shift" (0 auto; rows of a row
 * block, log2 of the columns of a column block); "row_split" (-1 auto / 0 / 1:
 * skewed row lengths -- rows above "row_split_threshold" entries, default 128,
 * are multiplied apart from the rest), "blockwin" (-1 / 0 / 1: the block-window
 * kernel for skewed rows whose columns stay near the rows -- -1: timed against
 * the row split at setup, 1: whenever every row block's window of x fits LDS).
 * Unknown key or a value the kernels are not instantiated for:
 * SPAL_ERR_INVALID_ARGUMENT. */
int spal_csr_set_option(spal_csr_t a, const char *key, int64_t value);
/* Setup-time autotune: runs the planned kernel's variants (the stream kernel
 * with one workgroup per super-tile vs. its walking form -- the sliding-window
 * kernel on band-like plans, else the persistent form -- each with plain or
 * non-temporal y stores; the column-blocked kernel against the stream kernels
 * where the plan built both) `iters` times each on the caller's device vectors
 * and keeps the fastest; then copies the 16-bit column array into
 * "place_tries" (default 8; up to three times as many while none is 3 % better)
 * blocks of 1 GiB taken one after the other from the
 * device's memory and keeps the place where the kernel ran fastest (two streams
 * out of one class of region disturb each other).  All variants
 * produce identical y.  Synchronises `stream`.  Cost at config 3 with
 * iters = 30: 0.1 ... 0.15 s. */
int spal_csr_autotune_f64(spal_csr_t a, const double *x_dev, double *y_dev,
                          void *stream, int iters);
int spal_csr_autotune_f32(spal_csr_t a, const float *x_dev, float *y_dev,
                          void *stream, int iters);
/* Device vectors x (ncols elements) and y (nrows elements) for products with THIS handle, placed so that the stores
 * of y do not collide with the matrix stream.  Why: on MI355X the time of a product depends on where y lies in the
 * device's memory RELATIVE to the matrix arrays (streams out of one class of region disturb each other: +-5 % at
 * config 3) -- a property of the pair that neither side can fix alone, and `hipMalloc` gives no say.
 * The FIRST such call in a process (per device) walks the device's memory in blocks of 1 GiB ("walk_blocks", default 8 =
 * at most 8 GiB held during the walk; ~3 ms each), times the handle's kernel into a candidate y in every block, KEEPS the
 * block where it ran fastest and -- when the walk met a second class of region -- the one where it ran slowest, as the
 * process's placement blocks, and frees the rest.  Every later call (any handle) only times the handle in the kept blocks
 * (two probes, no hipMalloc) and takes its vectors as a PIECE of the better one; spal_csr_autotune_* takes the 16-bit
 * columns from the same blocks.  Memory: at most two blocks of 1 GiB per process and device, shared by all handles
 * (spal_csr_describe: "placement_blocks", "placement_free_bytes"; a handle reports the new blocks its call took in
 * "vectors_walk_blocks" -- 0 once the process has its blocks -- and the places it timed in "vectors_probes").  The
 * vectors belong to the handle (their piece returns to the block with spal_csr_destroy; a second call returns the same
 * pointers); any other device memory works as x / y too, only possibly slower.  Matrices below 256 MB and handles above
 * 2^32 - 65537 entries (row blocks): a plain allocation of exactly the vectors' size.  Synchronises `stream`.
 * Replaces nothing in the reference: its `Vec<T>` has no placement.  Rust shim: `DeviceCsr::vectors()`. */
int spal_csr_alloc_vectors(spal_csr_t a, void **x_dev, void **y_dev, void *stream);
/* Writes a one-line JSON description of the active plan into buf: "kernel"
 * ("stream" | "vector"), "index_bits" (16: window-relative columns), the
 * geometry ("rows_per_tile", "rows_per_block", "lanes_per_row", ...),
 * "lds_window_bytes", "stream_row_fraction" (rows in tiles that stream),
 * "overflow_tiles" (tiles left to the overflow kernel), "skew", "persistent",
 * "slide", "ring_pages", "uniform_row_fraction", "nt_store", "autotune_us"
 * (one workgroup per super-tile, walking form, each then with non-temporal y
 * stores), "placement_us" (before / after placing the 16-bit columns),
 * "vectors_walk_us" (fastest / slowest block of spal_csr_alloc_vectors).
 * Plans with the sliding kernel add "rowrec", "rowrec_on",
 * "rowrec_bytes_per_row", "rowrec_max_span", "rowrec_failed", "rowrec_us" (the
 * autotune's {16-bit columns, records} per launch), and f64 handles among them
 * "valpack", "valpack_on", "valpack_bits" (of the widest k, sign included),
 * "valpack_exp" (e), "valpack_bytes_per_row", "valpack_failed", "valpack_us"
 * (the autotune's {values, packed values}), "valpack_build_ms". */
int spal_csr_describe(spal_csr_t a, char *buf, size_t buf_len);

/* ---- CSC: y = A * x (atomic scatter) --------------------------------------
 * Replaces `&a * &x_as_matrix` for `impl Mul for &CscMatrix<T>`
 * (src/csc/ops/mul.rs:5-60); bound as `impl Mul<&[T]> for &CscMatrix<T>`. */
int spal_csc_create_f64(int device, uint64_t nrows, uint64_t ncols,
                        const uint64_t *colptr, uint64_t colptr_len,
                        const uint64_t *rowind, uint64_t rowind_len,
                        const double *values, uint64_t values_len,
                        spal_csc_t *out);
int spal_csc_create_f32(int device, uint64_t nrows, uint64_t ncols,
                        const uint64_t *colptr, uint64_t colptr_len,
                        const uint64_t *rowind, uint64_t rowind_len,
                        const float *values, uint64_t values_len,
                        spal_csc_t *out);
int spal_csc_destroy(spal_csc_t a);
int spal_csc_shape(spal_csc_t a, uint64_t *nrows, uint64_t *ncols,
                   uint64_t *nnz, int *elem_size);
int spal_csc_spmv_f64(spal_csc_t a, const double *x, uint64_t x_len,
                      double *y, uint64_t y_len);
int spal_csc_spmv_f32(spal_csc_t a, const float *x, uint64_t x_len,
                      float *y, uint64_t y_len);
int spal_csc_spmv_dev_f64(spal_csc_t a, const double *x_dev, double *y_dev,
                          void *stream);
int spal_csc_spmv_dev_f32(spal_csc_t a, const float *x_dev, float *y_dev,
                          void *stream);
int spal_csc_download_f64(spal_csc_t a, uint64_t *colptr, uint64_t *rowind,
                          double *values);
int spal_csc_download_f32(spal_csc_t a, uint64_t *colptr, uint64_t *rowind,
                          float *values);
/* Keys: "kernel" 1 = atomic scatter (over ROW tiles where every tile's window
 * of x fits LDS beside its rows -- a workgroup owns rows of y, nothing is shared
 * between workgroups or launches; "row_tiles" -1 auto / 0 / 1 --, else over
 * column tiles: LDS-privatised where the row window of a
 * 1024-column block fits LDS, global atomics otherwise), 2 = transposed: the
 * matrix is converted to CSR on the device once and the CSR kernels run
 * (deterministic; bit-identical to the reference's k-ascending order), 0 = auto
 * (= 2).  "lds" 0/1, "cols_per_block" (0 auto / 1024 / 2048 / 4096 columns per
 * super-tile), "flush" tune kernel 1's column tiles (a flush other than 0 also
 * selects them).  flush 0 (default): where the super-tiles'
 * row windows ascend and overlap their neighbours' only (bands), every row of y
 * is stored by the first super-tile that covers it and completed by the next one
 * behind a flag -- no zero fill of y, no global atomics; launches of one handle
 * are then chained by an event (any streams), and on a stream that is being
 * captured into a graph the atomics form runs instead.  Otherwise, or with flush
 * 2: y is zeroed and window rows are added with global atomics.  flush 1: windows
 * stored per super-tile, then an ordered reduce.  spal_csc_describe reports the
 * form in "flush". */
int spal_csc_set_option(spal_csc_t a, const char *key, int64_t value);
/* as spal_csr_autotune_* for the transposed route (kernel 2); no-op for kernel 1 */
int spal_csc_autotune_f64(spal_csc_t a, const double *x_dev, double *y_dev,
                          void *stream, int iters);
int spal_csc_autotune_f32(spal_csc_t a, const float *x_dev, float *y_dev,
                          void *stream, int iters);
int spal_csc_describe(spal_csc_t a, char *buf, size_t buf_len);
/* Health of the device-pointer products (spal_csc_spmv_dev_*) issued so far; call it after synchronising their stream.
 * *invalid_products = products of this handle whose neighbour hand-off (kernel 1 over column tiles, flush 0) hit its
 * spin bound: their y was NOT valid.  The library also reports such a product by failing the NEXT product on the
 * handle (SPAL_ERR_HIP) and flushes with atomics from then on; a caller whose last product it was learns it here.
 * Always 0 for the transposed route, the row tiles and the atomics forms (nothing is handed over there).
 * Stream lifetime with the hand-off form: the handle remembers the stream of its last product and, when the next product
 * comes on ANOTHER stream, records an event on the remembered one -- so a stream that carried a product of this handle
 * must stay alive until the handle has been used on another stream or destroyed (or use one stream per handle). */
int spal_csc_status(spal_csc_t a, int *invalid_products);

/* ---- Y = A * X for a dense block of k vectors (SpMM), CSR and CSC --------------------
 * `&A * &X` of src/csr/ops/mul.rs:5-59 with every entry of X stored.  X is ncols x k, Y is nrows x k, both dense
 * and ROW-MAJOR: element (i, j) at [i * ld + j], ld >= k (so the k values a stored entry A[i,c] needs, X[c, 0..k),
 * are contiguous; a C-contiguous numpy / torch 2-D array is this layout with ld = k).  k * ld offsets are 64-bit.
 * Value of Y[i,j]: the stored entries of row i taken in ascending column, the first product ASSIGNED, every later
 * one added; multiply and add rounded separately (no FMA), in the operand type (f32 in f32); a row without stored
 * entries gives +0.0.  That is bit for bit the reference's Mul for a fully stored X.  No float atomics, no tree
 * reduction: the result is deterministic and does not depend on k, on ldx / ldy or on the column tile that ran.
 * (spal_csr_spmv_* promises those bits on its streaming kernels only: with one or two vectors spmv is the faster
 * call, with four or more spmm is -- the library never reroutes one to the other.)
 * Every element Y[i, 0..k) of every row is overwritten; the padding Y[i, k..ldy) is not touched.  X and Y must not
 * overlap.  No alignment of the pointers or leading dimensions beyond the element's own is needed.
 * SPAL_ERR_INVALID_ARGUMENT before any device work: null handle or pointers; k == 0; ldx < k or ldy < k; the host
 * form: x_rows != ncols ("assertion failed: ncols == rhs.nrows (left: .., right: ..)", mul.rs:9) or
 * y_rows != nrows; an _f64 entry on an f32 handle or the reverse.
 * k is not limited: a block wider than the column tile is covered by several tiles inside ONE pass over the matrix.
 * Row-block handles (more entries than 32-bit offsets address) are supported: block b writes its own rows of Y.
 * The kernel reads the handle's row pointers, 32-bit columns and values only: it needs nothing from the SpMV plan
 * and does not build it, so on a handle assembled on the device it may be the first call, also on a stream that is
 * being captured into a graph (the _dev forms allocate nothing and synchronise nothing).
 * The _dev forms are safe for concurrent calls on one handle (read-only on the matrix, no scratch memory); the host
 * forms serialise on the handle.
 * CSC handles run on their CSR twin (the one the default "kernel" = 2 product uses, built on the device on first
 * use) whatever "kernel" says for SpMV -- hence the same bits as CSR.  The atomic scatter routes have no SpMM form;
 * on a "kernel" = 1 handle the first SpMM builds the twin and therefore cannot be captured into a graph.
 * Option "spmm_tile" (spal_csr_set_option / spal_csc_set_option): the column tile KT -- a wave is 64 / KT rows x KT
 * columns of X.  0 = automatic (the narrowest tile that holds k, at most 32), else one of
 * 1, 2, 4, 8, 16, 32; anything else SPAL_ERR_INVALID_ARGUMENT.  After the first SpMM the handle's describe() line
 * carries an "spmm" object: tile and k of the last call, its column tiles, rows of a workgroup, long rows (rows a
 * whole wave walks, apart from the tiles). */
int spal_csr_spmm_f64(spal_csr_t a, uint64_t k, const double *x, uint64_t ldx, uint64_t x_rows,
                      double *y, uint64_t ldy, uint64_t y_rows);                 /* host arrays: H2D, kernel, D2H */
int spal_csr_spmm_f32(spal_csr_t a, uint64_t k, const float *x, uint64_t ldx, uint64_t x_rows,
                      float *y, uint64_t ldy, uint64_t y_rows);
int spal_csr_spmm_dev_f64(spal_csr_t a, uint64_t k, const double *x_dev, uint64_t ldx,
                          double *y_dev, uint64_t ldy, void *stream);            /* enqueued, not synchronised */
int spal_csr_spmm_dev_f32(spal_csr_t a, uint64_t k, const float *x_dev, uint64_t ldx,
                          float *y_dev, uint64_t ldy, void *stream);
int spal_csc_spmm_f64(spal_csc_t a, uint64_t k, const double *x, uint64_t ldx, uint64_t x_rows,
                      double *y, uint64_t ldy, uint64_t y_rows);
int spal_csc_spmm_f32(spal_csc_t a, uint64_t k, const float *x, uint64_t ldx, uint64_t x_rows,
                      float *y, uint64_t ldy, uint64_t y_rows);
int spal_csc_spmm_dev_f64(spal_csc_t a, uint64_t k, const double *x_dev, uint64_t ldx,
                          double *y_dev, uint64_t ldy, void *stream);
int spal_csc_spmm_dev_f32(spal_csc_t a, uint64_t k, const float *x_dev, uint64_t ldx,
                          float *y_dev, uint64_t ldy, void *stream);

/* ---- L x = b, U x = b: sparse triangular solve, CSR and CSC --------------------------
 * Not in the reference (it has no solve, as it has no SpMV); the contract is this sequential loop, which the device
 * reproduces bit for bit in f32 and f64 (NaN by position).  A is square and stored as the handle stores it, columns
 * strictly ascending inside a row.  `uplo` (0 lower, 1 upper) selects the triangle that is used; entries of the other
 * triangle are ignored, so a full matrix can be swept as it is (Gauss-Seidel, SSOR, an ILU factor stored in one matrix).
 *   lower, rows i = 0 .. n-1 (upper: i = n-1 .. 0, entries with j > i):
 *     s = b[i]
 *     for each stored (i, j, v) with j < i, in ascending column:  s = s - (v * x[j])   -- product rounded, then the
 *                                                                  difference: no FMA
 *     x[i] = s / d   (d = the stored (i, i) entry; IEEE division)      unit_diag = 1: x[i] = s, a stored (i, i) ignored
 * A stored zero diagonal is not an error: the result is what the division gives (inf / NaN, propagating).
 * SPAL_ERR_INVALID_ARGUMENT: A not square; unit_diag = 0 and some row stores no (i, i) entry (the message names the
 * first such row); uplo or unit_diag outside {0, 1}; null pointers; wrong lengths; an _f64 entry on an f32 handle or
 * the reverse.  SPAL_ERR_UNSUPPORTED: a handle held as row blocks (more than 2^32 - 65537 entries).
 *
 * spal_trsv_levels is the analysis, host only: level_of[i] = 0 when row i uses no off-diagonal entry of the chosen
 * triangle, else 1 + the largest level_of[j] over the entries it uses; *nlevels = 1 + the largest level (0 for n = 0).
 * One sequential O(nnz) pass.  A stored column >= n ("not square") and, with unit_diag = 0, a missing diagonal are
 * refused as above.
 *
 * On a handle there is one plan per triangle, built by the first solve of that triangle or by spal_*_trsv_analyse:
 * the row pointers and columns are copied back from the device (handles keep no host arrays), analysed on the host,
 * and the rows uploaded ordered by level -- this synchronises `stream` and allocates; its cost is "analysis_ms" of
 * describe().  Every later solve of that triangle allocates nothing and synchronises nothing: it enqueues the plan's
 * recorded launches on the caller's stream (the host forms copy b up, solve in place, copy x back and synchronise).
 * Rows of one level are independent and levels are ordered BY STREAM ORDER ONLY: a level wider than the option
 * "trsv_chain_rows" is one launch (a thread per row); every maximal run of consecutive narrower levels is one launch of
 * one workgroup that walks them with a barrier in between.  Nothing waits on another workgroup, so a solve cannot hang.
 * "trsv_chain_rows" (spal_csr_set_option / spal_csc_set_option, >= 0): 0 = every level its own launch, a huge value =
 * one launch for the whole solve; the bits do not depend on it.  Default 256.
 * x_dev == b_dev is allowed (in place); otherwise b is not written and the two must not overlap partially.
 * Calls on one handle serialise on the handle's lock (plan creation included), from any number of threads.
 * CSC handles solve on their CSR twin (built on the device on first use), so the definition holds unchanged.
 * GRAPH CAPTURE.  The first solve of a triangle (spal_*_trsv_dev_*, spal_*_trsm_dev_*) and spal_*_trsv_analyse on a
 * stream that is being captured are refused before any device work -- SPAL_ERR_INVALID_ARGUMENT, "... cannot be captured
 * into a graph: call spal_*_trsv_analyse for this triangle (or run one solve of it) before the capture" -- and the caller's
 * capture stays valid: building the plan allocates, copies to the host and synchronises.  A solve of a triangle that has
 * its plan is kernels only and is capturable (L then U in place is the application of an ILU(0) factor inside a captured
 * loop); once the plan exists the stream is not asked.
 * describe() gains "trsv": {"analyses": plans built, "lower" / "upper": {levels, max_level_rows, launches,
 * chain_launches, chain_rows, analysis_ms}} once a triangle was analysed. */
int spal_trsv_levels(uint64_t n, const uint64_t *rowptr, const uint64_t *colind, int uplo, int unit_diag,
                     uint64_t *level_of, uint64_t *nlevels);
int spal_csr_trsv_analyse(spal_csr_t a, int uplo, int unit_diag, void *stream);
int spal_csr_trsv_f64(spal_csr_t a, int uplo, int unit_diag, const double *b, uint64_t b_len,
                      double *x, uint64_t x_len);                                /* host vectors */
int spal_csr_trsv_f32(spal_csr_t a, int uplo, int unit_diag, const float *b, uint64_t b_len,
                      float *x, uint64_t x_len);
int spal_csr_trsv_dev_f64(spal_csr_t a, int uplo, int unit_diag, const double *b_dev, double *x_dev,
                          void *stream);                                         /* enqueued, not synchronised */
int spal_csr_trsv_dev_f32(spal_csr_t a, int uplo, int unit_diag, const float *b_dev, float *x_dev,
                          void *stream);
int spal_csc_trsv_analyse(spal_csc_t a, int uplo, int unit_diag, void *stream);
int spal_csc_trsv_f64(spal_csc_t a, int uplo, int unit_diag, const double *b, uint64_t b_len,
                      double *x, uint64_t x_len);
int spal_csc_trsv_f32(spal_csc_t a, int uplo, int unit_diag, const float *b, uint64_t b_len,
                      float *x, uint64_t x_len);
int spal_csc_trsv_dev_f64(spal_csc_t a, int uplo, int unit_diag, const double *b_dev, double *x_dev,
                          void *stream);
int spal_csc_trsv_dev_f32(spal_csc_t a, int uplo, int unit_diag, const float *b_dev, float *x_dev,
                          void *stream);

/* ---- Jacobi sweeps on a triangle: an approximate L x = b / U x = b in s SpMV-shaped passes -------------
 * Not in the reference.  The exact solve above is a chain of levels ordered by the stream, and the chain is a property
 * of the matrix (8028 levels per triangle on the banded 1M x 1M factor).  A preconditioner does not need
 * the exact solve: sweep(A, uplo, unit_diag, s, b) -> x replaces it by s Jacobi passes x <- D^-1 (b - N x) on the chosen
 * triangle (N: the triangle off the diagonal), every pass one launch in which all rows are independent.  It gives up
 * exactness of the SOLVE, not of the arithmetic: the contract is again a sequential text that the device reproduces bit
 * for bit in f32 and f64 (NaN by position), T the handle's element type:
 *   d[i]  = the stored (i, i) entry                      (unit_diag = 1: not read)
 *   x0[i] = b[i] / d[i]                                  (unit_diag = 1: b[i])
 *   for t = 1 .. s, every row i independently of the others:
 *       acc = b[i]
 *       for each stored (i, j, v) of the chosen triangle off the diagonal, in ascending column:
 *           acc = acc - (v * x(t-1)[j])      -- product rounded, then the difference: no FMA
 *       xt[i] = acc / d[i]                                (unit_diag = 1: acc)
 *   result: xs
 * Triangle selection (`uplo` 0: entries with j < i, 1: j > i), IEEE division and the errors are the exact solve's:
 * SPAL_ERR_INVALID_ARGUMENT for A not square, unit_diag = 0 and a row without a stored (i, i) (the message names the
 * first such row), flags outside {0, 1}, null pointers, wrong lengths, an _f64 entry on an f32 handle or the reverse;
 * SPAL_ERR_UNSUPPORTED for a handle held as row blocks.  A stored zero diagonal is not an error (inf / NaN, propagating).
 * Entries of the other triangle are ignored and their values never enter the arithmetic (they may be NaN).
 * Two consequences:
 *   EQUALITY WITH THE EXACT SOLVE.  A row of level l (as spal_trsv_levels defines it) holds its final value from x_l on,
 *   NaN positions included: by induction the rows it reads, of levels < l, are final in x(l-1), so pass l performs the
 *   operations of the sequential substitution on the same inputs, and so does every later pass.  Hence for
 *   s >= nlevels - 1 the result is bit for bit that of spal_*_trsv_*.
 *   CLAMPING.  nlevels <= n, so an s greater than n - 1 is clamped to n - 1 without changing a bit: a call enqueues at
 *   most n launches whatever `sweeps` is.
 * s = 0 on A itself is the Jacobi preconditioner D^-1 b.
 * Preparation: a sweep needs, per row, the position of its first entry with column >= row and whether that is the
 * diagonal.  One small kernel builds this on the first sweep call of a handle (under the handle's lock; it synchronises
 * `stream` once to read back the first row without a diagonal).  There is no host analysis and no solve plan: after
 * sweep calls alone describe() shows no "trsv" object.  Every later call allocates no handle state and synchronises
 * nothing: x0 is one launch, every pass one more, ordered by the stream alone -- no atomics, no flags, nothing waits on
 * another workgroup, so a call cannot hang.  The host forms copy b up, sweep, copy x back and synchronise.  The _dev
 * forms enqueue on `stream`; x_dev == b_dev is allowed (a row reads only its own b[i]); the passes ping-pong through
 * scratch: none for s = 0, one vector for s = 1, two beyond.  SCRATCH IS PER STREAM (as for spal_dot_dev_*): the library
 * keeps one block per (device, stream), taken from the runtime's stream-ordered allocator on that stream by the first call
 * that needs one, grown the same way by a call that needs more, and reused by every later call on that stream, which
 * therefore makes no allocator call and does not wait for the stream however busy it is.  Calls on one stream use the
 * block one after the other in stream order; two calls on different streams never share scratch.  hipStreamPerThread,
 * one handle value for a different stream in every thread, is served by a block of the call's own, taken and returned
 * in stream order per call (on a busy stream the runtime's hipFreeAsync may then wait on the host).  Nothing is asked
 * of the caller: a handle value that names a new stream after hipStreamDestroy is ordered behind the block's last user
 * by an event.  The blocks stay allocated until spal_cache_trim.
 * GRAPH CAPTURE.  The first sweep call of a handle -- of a vector or of a block -- on a stream that is being captured is
 * refused before any device work (SPAL_ERR_INVALID_ARGUMENT, "... cannot be captured into a graph: run one sweep call on
 * this handle ... before the capture"; the capture stays valid): the preparation allocates and synchronises.  On a
 * prepared handle s = 0 is kernels only and capturable.  s >= 1 on a capturing stream is refused in the same way ("...
 * takes scratch from the library's per-stream block: it cannot be captured into a graph ..."), and so is spal_dot_dev_*:
 * a graph would hold a block that the library may release.
 * CSC handles sweep on their CSR twin.  Calls on one handle serialise on its lock, from any number of threads.
 * describe() gains "trsv_sweep": {prepared, prepare_ms, block_rows = rows of a workgroup, chunk_entries = entries it
 * stages in LDS at a time, calls} once the handle is prepared.
 * Option "trsv_sweeps" (spal_csr_set_option / spal_csc_set_option on a factor, >= -1; default -1): read by
 * spal_*_krylov_* from its `m` only (below); the spal_*_trsv_* entry points ignore it and stay exact. */
int spal_csr_trsv_sweep_f64(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, const double *b, uint64_t b_len,
                            double *x, uint64_t x_len);                          /* host vectors */
int spal_csr_trsv_sweep_f32(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, const float *b, uint64_t b_len,
                            float *x, uint64_t x_len);
int spal_csr_trsv_sweep_dev_f64(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, const double *b_dev,
                                double *x_dev, void *stream);                    /* enqueued, not synchronised */
int spal_csr_trsv_sweep_dev_f32(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, const float *b_dev,
                                float *x_dev, void *stream);
int spal_csc_trsv_sweep_f64(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, const double *b, uint64_t b_len,
                            double *x, uint64_t x_len);
int spal_csc_trsv_sweep_f32(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, const float *b, uint64_t b_len,
                            float *x, uint64_t x_len);
int spal_csc_trsv_sweep_dev_f64(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, const double *b_dev,
                                double *x_dev, void *stream);
int spal_csc_trsv_sweep_dev_f32(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, const float *b_dev,
                                float *x_dev, void *stream);

/* ---- triangular solves for a block of k right-hand sides, exact and by sweeps, CSR and CSC -------------
 * Not in the reference.  B and X are n x k, dense and ROW-MAJOR: element (i, j) at [i * ld + j], ld >= k -- the layout
 * of spal_*_spmm_*; offsets i * ld are 64-bit.  One call solves all k columns on the launches of ONE single-vector call.
 *   EXACT (spal_*_trsm_*).  Column j of X is, bit for bit in f32 and f64 with NaN by position, what spal_*_trsv_*
 *   returns for column j of B: the sequential text above, applied per column.
 *   SWEEPS (spal_*_trsm_sweep_*).  Column j of X is, bit for bit, what spal_*_trsv_sweep_* returns for column j of B with
 *   the same `sweeps`.  From sweeps >= nlevels - 1 on these are the exact block solve's bits; an s > n - 1 is clamped to
 *   n - 1, so a call enqueues at most n launches.
 * INDEPENDENCE OF THE GEOMETRY.  A column's sum is never split and never meets another column's: the bits do not depend
 * on k, ldb, ldx, the column tile or "trsv_chain_rows".  A NaN or inf in one column of B never reaches another column.
 * PADDING.  X[i, 0..k) is overwritten for every row; the padding X[i, k..ldx) is not touched; the padding of B is never
 * read.  IN PLACE: x == b is allowed when ldx == ldb (element (i, j) is read before it is stored, and nothing else of B
 * is read); otherwise the two blocks must not overlap.
 * WIDTH.  k is not limited: a block wider than the column tile is covered inside each launch.  The exact solve enqueues
 * exactly the plan's recorded launches ("launches" of describe()["trsv"]) whatever k is, a sweep call exactly 1 + s;
 * column panels are never looped on the host.  Order between workgroups comes from the stream alone -- no flags, no
 * spins, no atomics, no grid syncs -- so a call cannot hang.
 * SPAL_ERR_INVALID_ARGUMENT before any device work: null handle or pointers; k == 0; ldb < k or ldx < k; x == b with
 * ldx != ldb; the host forms: b_rows != nrows or x_rows != nrows; uplo or unit_diag outside {0, 1}; an _f64 entry on an
 * f32 handle or the reverse; a matrix that is not square; unit_diag = 0 and a row without a stored (i, i) (the message
 * names the first such row).  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.
 * THE PLAN IS THE VECTOR SOLVE'S.  The first exact solve of a triangle -- of a vector or of a block -- builds the
 * triangle's plan, which synchronises `stream`; every later call, of either kind, allocates nothing and synchronises
 * nothing, and "analyses" of describe()["trsv"] stays 1.  The sweep forms use the handle's sweep preparation, built by
 * the first sweep call of either kind (no host analysis, no plan); their ping-pong scratch is n * k elements per buffer
 * -- none for s = 0, one buffer for s = 1, two beyond -- in the stream's own scratch block, as the single-vector form
 * has it.  GRAPH CAPTURE is the vector forms': a first exact solve of a triangle and a first sweep call are refused
 * inside a capture (analyse or prepare before), a planned exact solve and an s = 0 sweep on a prepared handle are
 * capturable, s >= 1 on a capturing stream is refused.  The host forms copy B up packed, solve in place, copy
 * the k columns of X back and synchronise.  CSC handles run on their CSR twin.  Calls on one handle serialise on its
 * lock, as the vector solves do.
 * Option "trsm_tile" (spal_csr_set_option / spal_csc_set_option): the column tile KT -- a wave is 64 / KT rows x KT
 * columns of X.  0 = automatic (the narrowest tile that holds k, at most 32), else one of 1, 2, 4, 8, 16, 32; anything
 * else SPAL_ERR_INVALID_ARGUMENT.  After the first block call describe() carries a "trsm" object: {tile, k,
 * column_tiles, launches} of the last call, and calls / sweep_calls, the exact and the sweep calls so far. */
int spal_csr_trsm_f64(spal_csr_t a, int uplo, int unit_diag, uint64_t k, const double *b, uint64_t ldb,
                      uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows);
int spal_csr_trsm_dev_f64(spal_csr_t a, int uplo, int unit_diag, uint64_t k, const double *b_dev, uint64_t ldb,
                          double *x_dev, uint64_t ldx, void *stream);
int spal_csr_trsm_sweep_f64(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k, const double *b,
                            uint64_t ldb, uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows);
int spal_csr_trsm_sweep_dev_f64(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k,
                                const double *b_dev, uint64_t ldb, double *x_dev, uint64_t ldx, void *stream);
int spal_csr_trsm_f32(spal_csr_t a, int uplo, int unit_diag, uint64_t k, const float *b, uint64_t ldb,
                      uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows);
int spal_csr_trsm_dev_f32(spal_csr_t a, int uplo, int unit_diag, uint64_t k, const float *b_dev, uint64_t ldb,
                          float *x_dev, uint64_t ldx, void *stream);
int spal_csr_trsm_sweep_f32(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k, const float *b,
                            uint64_t ldb, uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows);
int spal_csr_trsm_sweep_dev_f32(spal_csr_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k,
                                const float *b_dev, uint64_t ldb, float *x_dev, uint64_t ldx, void *stream);
int spal_csc_trsm_f64(spal_csc_t a, int uplo, int unit_diag, uint64_t k, const double *b, uint64_t ldb,
                      uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows);
int spal_csc_trsm_dev_f64(spal_csc_t a, int uplo, int unit_diag, uint64_t k, const double *b_dev, uint64_t ldb,
                          double *x_dev, uint64_t ldx, void *stream);
int spal_csc_trsm_sweep_f64(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k, const double *b,
                            uint64_t ldb, uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows);
int spal_csc_trsm_sweep_dev_f64(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k,
                                const double *b_dev, uint64_t ldb, double *x_dev, uint64_t ldx, void *stream);
int spal_csc_trsm_f32(spal_csc_t a, int uplo, int unit_diag, uint64_t k, const float *b, uint64_t ldb,
                      uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows);
int spal_csc_trsm_dev_f32(spal_csc_t a, int uplo, int unit_diag, uint64_t k, const float *b_dev, uint64_t ldb,
                          float *x_dev, uint64_t ldx, void *stream);
int spal_csc_trsm_sweep_f32(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k, const float *b,
                            uint64_t ldb, uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows);
int spal_csc_trsm_sweep_dev_f32(spal_csc_t a, int uplo, int unit_diag, uint64_t sweeps, uint64_t k,
                                const float *b_dev, uint64_t ldb, float *x_dev, uint64_t ldx, void *stream);

/* ---- ILU(0): the incomplete LU factorisation without fill, CSR and CSC ------------------
 * Not in the reference; the contract is this sequential loop, which the device reproduces bit for bit in f32 and f64
 * (NaN by position).  A is square and stored as the handle stores it, columns strictly ascending inside a row, and every
 * row stores its (i, i) entry.  F starts as a copy of A's values; its structure is A's and never changes (no fill).
 *   for i = 0 .. n-1:
 *     for each stored (i, k) with k < i, in ascending k, at position p:
 *       w = F[p] / F[diag(k)]                 -- IEEE division; row k is final
 *       F[p] = w
 *       for each stored (k, j) with j > k, in ascending j, value u = F[(k, j)]:
 *         if (i, j) is stored, at position q:  F[q] = F[q] - (w * u)   -- product rounded, then the difference: no FMA
 * The result is a new, independent handle of a's shape, structure and element type (type-generic, like spal_csr_neg)
 * that holds L strictly below the diagonal, its unit diagonal implied, and U on and above the diagonal.  M^-1 r is
 * therefore two solves on that one handle: spal_*_trsv(uplo = 0, unit_diag = 1) for L y = r, then
 * spal_*_trsv(uplo = 1, unit_diag = 0) for U z = y.  A zero or non-finite pivot is not an error: the result is what the
 * division gives, propagating.  `a` is only read.
 * SPAL_ERR_INVALID_ARGUMENT: null arguments; A not square; a row without a stored diagonal (the message names the first
 * such row).  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  Nothing leaks on failure and *out is not written.
 * The schedule is the lower solve's (row i needs exactly the rows k < i it stores): the call builds a's lower solve plan
 * if a has none (counted in a's "analyses"), walks its launch list -- "trsv_chain_rows" governs both -- and
 * synchronises `stream`.  The result's product plan is lazy (nobody multiplies by L\U); it receives a copy of a's lower
 * solve plan, so its first lower solve analyses nothing; its upper plan is built by its first upper solve.
 * A row is factorised by one thread, or, when the updates it has to look for (the sum, over its k, of the entries of
 * row k past the diagonal) number at least the option "ilu_wide_work" (spal_csr_set_option / spal_csc_set_option,
 * >= 0; 0 = every row with an entry below the diagonal, a huge value = none), by one wave whose lanes spread over row
 * k; the bits do not depend on it.  CSC handles factorise their CSR twin and return the factor as CSC.
 * describe() on the result gains "ilu0": {levels, launches, chain_launches, rows_row_form, rows_wide_form, wide_work,
 * chain_rows, lds_stage_entries, kernel_ms = device time of the kernels, call_ms}. */
int spal_csr_ilu0(spal_csr_t a, void *stream, spal_csr_t *out);
int spal_csc_ilu0(spal_csc_t a, void *stream, spal_csc_t *out);

/* ---- ILU(0) by row sweeps: the factor in s SpMV-shaped passes, no analysis ------------------
 * Not in the reference.  The fine-grained ILU idea (Chow and Patel) in the form that is the factorisation's twin of
 * spal_*_trsv_sweep_*: again a sequential text that the device reproduces bit for bit in f32 and f64 (NaN by position).
 * A is as for ILU(0): square, columns ascending inside a row, every row stores (i, i).  T is the handle's element type.
 *   F0 = A's values
 *   for t = 1 .. s, every row i independently of the others:
 *       row i of Ft starts as a copy of row i of A
 *       for each stored (i, k) with k < i, in ascending k, at position p:
 *           w = Ft[p] / F(t-1)[diag(k)]                    -- IEEE division
 *           Ft[p] = w
 *           for each stored (k, j) with j > k, in ascending j, value u = F(t-1)[(k, j)]:
 *               if (i, j) is stored, at position q:  Ft[q] = Ft[q] - (w * u)   -- product rounded, then the difference: no FMA
 *   result: Fs   (s = 0: A's values on A's structure)
 * This is the body of ILU(0)'s loop for row i with every read of ANOTHER row taken from the previous pass; the row's own
 * running values are this pass's.  Three consequences:
 *   EQUALITY WITH ILU(0).  A row of level l of the lower triangle (as spal_trsv_levels defines it) holds its final bits
 *   from F_l on, NaN positions included: level-0 rows have no entry below the diagonal, so they are A's rows in every
 *   pass; by induction the rows k that a level-l row reads are final in F(l-1), so pass l performs the sequential loop's
 *   operations on the same inputs, and so does every later pass.  Hence for s >= nlevels - 1 the result is bit for bit
 *   that of spal_*_ilu0.
 *   CLAMPING.  nlevels <= n, so an s greater than n - 1 is clamped to n - 1 without changing a bit: a call enqueues at
 *   most n - 1 passes whatever `sweeps` is.
 *   APPROXIMATION.  A smaller s gives up exactness of the factor, not of the arithmetic: the result is still this text's,
 *   bit for bit, and it is a preconditioner in its own right (DESIGN 3.19 has the measured iteration counts).
 * The result has the shape of spal_*_ilu0's: a new, independent handle of a's structure and element type, L strictly
 * below the diagonal (unit diagonal implied) and U on and above it, with a lazy product plan.  The errors and their
 * messages are spal_*_ilu0's; *out is not written and nothing leaks.  `a` is only read; the call synchronises `stream`
 * once, at its end.
 * NO HOST ANALYSIS, NO SOLVE PLAN.  The diagonals' positions come from the preparation spal_*_trsv_sweep_* builds per
 * handle (one kernel, on first use, under the handle's lock; it names the first row without a diagonal): a's describe()
 * shows "analyses" unchanged and no "trsv" object it did not have.  The factor receives no solve plan: it is meant to be
 * applied by sweeps ("trsv_sweeps", spal_*_trsv_sweep_*); an exact solve on it analyses as usual.
 * One pass is one launch (one more, before the first, classifies the rows); order between passes is stream order alone:
 * no atomics on values, no flags, nothing waits on another workgroup.  The passes ping-pong between the result's values
 * and one scratch array from the runtime's stream-ordered allocator, the parity chosen so that the last pass lands in
 * the result: s = 0 is a copy, s = 1 needs no scratch, pass 1 reads A's array as F0.  Concurrent calls on one handle
 * share nothing but the preparation.
 * A workgroup owns block_rows consecutive rows and stages their entries in LDS when they number at most stage_entries
 * (else those rows run in place in the pass's output); a row is factorised by one thread or, from "ilu_wide_work"
 * updates to look for (the option of spal_*_ilu0, read from a), by one wave, staged in LDS up to wide_stage_entries
 * entries and in place beyond.  The bits depend on none of this.  CSC handles factorise their CSR twin and return the
 * factor as CSC.
 * describe() on the result gains "ilu0_sweep": {sweeps = passes run (after clamping), requested, launches = passes,
 * block_rows, stage_entries, wide_stage_entries, rows_row_form, rows_wide_form, wide_work, kernel_ms = device time,
 * call_ms}; it has no "ilu0" object. */
int spal_csr_ilu0_sweep(spal_csr_t a, uint64_t sweeps, void *stream, spal_csr_t *out);
int spal_csc_ilu0_sweep(spal_csc_t a, uint64_t sweeps, void *stream, spal_csc_t *out);

/* ---- A x = b on the device: CG and BiCGStab, optionally preconditioned by an ILU(0) factor ------------
 * Not in the reference.  As for the solve and the factorisation, the contract is a sequential text that the device
 * reproduces bit for bit in f32 and f64; a Krylov loop can only keep that promise if its reductions have ONE order, so
 * the dot product is defined first and everything below is built from it.
 *
 * dot(a, b, n), element type T:  p[i] = a[i] * b[i], each product rounded; the result is reduce(p).
 * reduce(v), v of length m:  c = max(1, ceil(m / 1024)); v is padded with +0.0 to 1024 * c elements (the zeros ARE
 *   added: a lone -0.0 gives +0.0, n = 0 gives +0.0); in every tile of 1024 consecutive elements, for h = 512, 256, ..,
 *   1:  e[t] = e[t] + e[t + h] for t < h, and the tile's sum is e[0]; c == 1: that sum is the result, otherwise the
 *   result is reduce(the c tile sums in order).  NaN propagates by IEEE.  The definition depends on n alone -- not on
 *   a grid, a wave size or the number of launches.
 * spal_dot_* restate it on the host (no device needed, like spal_trsv_levels); spal_dot_dev_* enqueue it on `stream`
 * for device vectors and write the one result to out_dev: not synchronised (tile sums go through the stream's own
 * scratch block, kept per (device, stream) as described with spal_*_trsv_sweep_dev_*: a call on a stream that has its
 * block allocates nothing and does not wait for the stream; on a capturing stream the call is refused).
 *
 * The two loops.  All scalars are T.  thr = T(tol * tol) * bb with bb = dot(b, b) (tol is a double; tol * tol is formed
 * in double and rounded to T once).  x holds x0 on entry and the result on exit.  M^-1 v with a factor handle m is
 * trsv(m, lower, unit_diag = 1) followed by trsv(m, upper, unit_diag = 0); with m == NULL it is v itself.  When m's
 * option "trsv_sweeps" is s >= 0, M^-1 v is instead sweep(m, lower, unit_diag = 1, s, v) followed by
 * sweep(m, upper, unit_diag = 0, s, .) -- the sweeps defined above, wherever "M^-1" stands in the two loops; -1, the
 * default, means the exact solves.  M = A with "trsv_sweeps" = 0 is the Jacobi preconditioner: the lower sweep with a
 * unit diagonal copies v, the upper one divides by the stored diagonal.  Every product alpha * v[i] is rounded before
 * the sum it enters (no FMA).
 *   test (on rr):  rr <= thr: stop, reason 0;  else rr not finite: stop, reason 2;  else it == maxit: stop, reason 1.
 *   Nothing is an error because of values: a breakdown (a zero denominator, an overflow) shows as reason 2.
 *
 *   SPAL_KRYLOV_CG
 *     q = A x;  r[i] = b[i] - q[i];  rr = dot(r, r);  it = 0;  test
 *     z = M^-1 r;  p = z;  rz = dot(r, z)
 *     while not stopped:
 *       q = A p;  alpha = rz / dot(p, q)
 *       x[i] = x[i] + (alpha * p[i]);  r[i] = r[i] - (alpha * q[i]);  it += 1
 *       rr = dot(r, r);  test
 *       z = M^-1 r;  rz1 = dot(r, z);  beta = rz1 / rz;  rz = rz1;  p[i] = z[i] + (beta * p[i])
 *
 *   SPAL_KRYLOV_BICGSTAB
 *     r = b - A x (as above);  rhat = r;  rho = alpha = omega = 1;  v = p = 0;  rr = dot(r, r);  it = 0;  test
 *     while not stopped:
 *       rho1 = dot(rhat, r);  beta = (rho1 / rho) * (alpha / omega);  rho = rho1
 *       p[i] = r[i] + (beta * (p[i] - (omega * v[i])))
 *       ph = M^-1 p;  v = A ph;  alpha = rho / dot(rhat, v)
 *       s[i] = r[i] - (alpha * v[i]);  it += 1
 *       ss = dot(s, s);  if ss <= thr (reason 0) or ss not finite (reason 2):
 *                            x[i] = x[i] + (alpha * ph[i]);  r = s;  rr = ss;  stop      -- the half-step exit
 *       sh = M^-1 s;  t = A sh;  omega = dot(t, s) / dot(t, t)
 *       x[i] = (x[i] + (alpha * ph[i])) + (omega * sh[i]);  r[i] = s[i] - (omega * t[i])
 *       rr = dot(r, r);  test
 *   (The half-step exit is part of the contract: with M = A exactly -- a diagonal or triangular A and its own factor --
 *   s is exactly zero and omega would be 0 / 0.)
 *
 * On the device the scalars live in a small block of device memory; the one-workgroup launch that finishes a dot also
 * does the scalar arithmetic that follows it, and every vector update is fused with the first level of the dot that
 * follows it -- neither changes a bit.  The host enqueues "krylov_check_every" iterations, then copies the status block
 * to pinned memory and synchronises.  Once the device has stopped, every later vector or scalar kernel of the call
 * reads the stop flag and writes nothing (products and solves still run, into work vectors), so x, iterations and
 * residual_sq are the values AT the stop whatever the poll interval is.  The flag is written by an earlier launch on
 * the same stream and only read: nothing waits on it, nothing spins.
 * Option "krylov_check_every" (spal_csr_set_option / spal_csc_set_option on `a`, >= 1; 0 is refused): default 8 without
 * a preconditioner and 1 with one.  The bits do not depend on it.
 * Before the first iteration the call builds a's product plan and m's lower and upper solve plans if they do not exist
 * yet (a first touch is fine; it synchronises) -- with "trsv_sweeps" >= 0 it prepares m for sweeps instead and
 * analyses no triangle -- and takes its work vectors from the caching allocator (two more for the sweeps' ping-pong,
 * so no iteration allocates); no handle lock is
 * held across a product or a solve (each takes its own), so calls on one handle from several threads are safe.
 * CSC handles multiply by their own SpMV route and solve on their CSR twin.  The _dev forms SYNCHRONISE `stream` (they
 * poll) and cannot be captured into a graph.
 * info: iterations, reason (0 converged, 1 maxit, 2 breakdown / not finite), residual_sq = rr and rhs_sq = bb (exact
 * conversions of the T values), solve_ms = device time from the first to the last launch of the call.
 * SPAL_ERR_INVALID_ARGUMENT: null a, b, x or info; wrong lengths (host forms); a or m not square; shapes, devices or
 * element types of a and m that differ, an _f64 entry on an f32 handle or the reverse; a method outside the enum; tol
 * negative or NaN; m with a row that stores no diagonal (the solve's own message); x_dev == b_dev.
 * SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  Nothing leaks on failure.
 * describe() on `a` gains "krylov" after a solve: {method, preconditioned, iterations, reason, check_every, polls,
 * solve_ms, precond_sweeps = m's "trsv_sweeps" (-1 without m)} of the last call.
 * Not provided: capture into a graph, several GPUs, a dot fused into the SpMV kernels.  GMRES has its own entry points
 * (below). */
enum { SPAL_KRYLOV_CG = 0, SPAL_KRYLOV_BICGSTAB = 1 };
typedef struct spal_krylov_info {
    uint64_t iterations;
    int reason;
    double residual_sq, rhs_sq, solve_ms;
} spal_krylov_info;
int spal_dot_f64(const double *a, const double *b, uint64_t n, double *out);      /* host only */
int spal_dot_f32(const float *a, const float *b, uint64_t n, float *out);
int spal_dot_dev_f64(int device, const double *a_dev, const double *b_dev, uint64_t n, double *out_dev,
                     void *stream);                                               /* enqueued, not synchronised */
int spal_dot_dev_f32(int device, const float *a_dev, const float *b_dev, uint64_t n, float *out_dev,
                     void *stream);
int spal_csr_krylov_f64(spal_csr_t a, int method, spal_csr_t m, const double *b, uint64_t b_len,
                        double *x, uint64_t x_len, double tol, uint64_t maxit,
                        spal_krylov_info *info);                                  /* host vectors; m NULL: none */
int spal_csr_krylov_f32(spal_csr_t a, int method, spal_csr_t m, const float *b, uint64_t b_len,
                        float *x, uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_krylov_dev_f64(spal_csr_t a, int method, spal_csr_t m, const double *b_dev, double *x_dev,
                            double tol, uint64_t maxit, void *stream,
                            spal_krylov_info *info);                              /* synchronises */
int spal_csr_krylov_dev_f32(spal_csr_t a, int method, spal_csr_t m, const float *b_dev, float *x_dev,
                            double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_krylov_f64(spal_csc_t a, int method, spal_csc_t m, const double *b, uint64_t b_len,
                        double *x, uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_krylov_f32(spal_csc_t a, int method, spal_csc_t m, const float *b, uint64_t b_len,
                        float *x, uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_krylov_dev_f64(spal_csc_t a, int method, spal_csc_t m, const double *b_dev, double *x_dev,
                            double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_krylov_dev_f32(spal_csc_t a, int method, spal_csc_t m, const float *b_dev, float *x_dev,
                            double tol, uint64_t maxit, void *stream, spal_krylov_info *info);

/* ---- A X = B on the device: CG and BiCGStab for a block of k right-hand sides --------------------------
 * Not in the reference.  ONE call runs k INDEPENDENT iterations in lockstep on shared launches: one pass over the
 * matrix per product and one walk of the factor's launches per solve serve all k columns.  It is not the block-Krylov
 * method with a shared search space: every column keeps its own sequential text, so the contract above carries over.
 * LAYOUT.  B and X are n x k, dense and ROW-MAJOR: element (i, j) at [i * ld + j], ld >= k -- the layout of
 * spal_*_spmm_* and spal_*_trsm_*; offsets i * ld are 64-bit.  X holds X0 on entry and the result on exit.
 * COLUMN j IS THE LOOP ABOVE.  Column j follows SPAL_KRYLOV_CG / SPAL_KRYLOV_BICGSTAB as written above, applied to
 * B[:, j] and X[:, j], with its own bb, thr, scalars, it, stop test, reason and residual_sq.  dot is the dot above
 * (tiles of 1024 rows) applied to the column.  A v is the value spal_*_spmm_* defines (ascending columns, the first
 * product assigned, no FMA: the reference's bits).  M^-1 v is column j of spal_*_trsm_*(lower, unit_diag = 1) followed
 * by spal_*_trsm_*(upper, unit_diag = 0); with m's option "trsv_sweeps" = s >= 0 it is column j of the two
 * spal_*_trsm_sweep_* calls with s sweeps; with m == NULL it is v.  Hence for every column x, iterations, reason,
 * residual_sq and rhs_sq are, bit for bit in f32 and f64, what the text gives -- and, on a handle whose SpMV runs a
 * sequential-order kernel, what spal_*_krylov_* returns for that column.  solve_ms is the call's device time, the same
 * in all k records.
 * WHAT THE BITS DO NOT DEPEND ON: k, ldb, ldx, the column tile, "krylov_check_every", what the other columns hold.  A
 * NaN, an inf or a breakdown in one column never reaches another.
 * FREEZE, PER COLUMN.  Once column j has stopped, no kernel writes its x, r, p, scalars or it again; BiCGStab's
 * half-step update is applied to exactly the columns that asked for it; the other columns go on.  The call ends when
 * every column has stopped, so maxit bounds it.  Products and solves keep running on all k columns, into work blocks:
 * the work on finished columns is wasted and accepted -- the active columns are not compacted.
 * PADDING.  X[i, k..ldx) is never written and B[i, k..ldb) is never read.  X and B must not overlap.
 * SPAL_ERR_INVALID_ARGUMENT before any device work: everything spal_*_krylov_* refuses (null a, b, x or info -- info
 * points to k records --, a or m not square, shapes, devices or element types of a and m that differ, an _f64 entry on
 * an f32 handle or the reverse, a method outside the enum, tol negative or NaN); k == 0; ldb < k or ldx < k; the host
 * forms: b_rows != nrows or x_rows != nrows; x_dev == b_dev.  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.
 * SPAL_ERR_OUT_OF_MEMORY: no room for the work blocks; nothing leaks.  The messages begin "spal_csr_krylov_block:" /
 * "spal_csc_krylov_block:".
 * The _dev forms SYNCHRONISE `stream` (they poll) and are refused on a capturing stream.  Before the first iteration
 * the call builds what spal_*_krylov_* builds (a's product plan; m's two solve plans, or its sweep preparation), takes
 * ALL its work blocks (3 / 4 for CG without / with m, 6 / 8 for BiCGStab, n x k each), the dots' scratch and the k
 * scalar records from the caching allocator in one go, and grows the stream's sweep scratch to n x k per buffer: no
 * iteration allocates, and nothing synchronises except the polls, which copy the k scalar records to pinned memory and
 * count the stopped columns.  No handle lock is held across a product or a solve, so calls on one handle from several
 * threads are safe.  Order between launches comes from the stream alone -- no flags waited on, no spins, no float
 * atomics, no grid syncs -- so a call cannot hang.  CSC handles multiply through their CSR twin, as SpMM does, and
 * solve on it.  The host forms copy B and X0 up packed, iterate, and copy the k columns of X back.
 * Options on `a`: "krylov_check_every" as above, same defaults and meaning.  "krylov_tile": the column tile KT of the
 * fused vector kernels -- a workgroup covers 1024 rows x KT columns, a wave reads 64 / KT rows x KT columns.  0 =
 * automatic (the narrowest tile that holds k, at most 32), else one of 1, 2, 4, 8, 16, 32; anything else
 * SPAL_ERR_INVALID_ARGUMENT.  A block wider than the tile is covered inside each launch.
 * describe() on `a` gains "krylov_block" after a call: {method, k, preconditioned, precond_sweeps, tile,
 * iterations_min, iterations_max, converged (columns that ended with reason 0), check_every, polls, solve_ms} of the
 * last call; "krylov" stays with the vector calls.
 * Not provided: compaction of finished columns, a true block-Krylov method (shared search space), capture into a
 * graph, several GPUs.  GMRES on a block has its own entry points below. */
int spal_csr_krylov_block_f64(spal_csr_t a, int method, spal_csr_t m, uint64_t k, const double *b, uint64_t ldb,
                              uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);                            /* host blocks; info: k records */
int spal_csr_krylov_block_f32(spal_csr_t a, int method, spal_csr_t m, uint64_t k, const float *b, uint64_t ldb,
                              uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);
int spal_csr_krylov_block_dev_f64(spal_csr_t a, int method, spal_csr_t m, uint64_t k, const double *b_dev,
                                  uint64_t ldb, double *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);                        /* synchronises; info on the host */
int spal_csr_krylov_block_dev_f32(spal_csr_t a, int method, spal_csr_t m, uint64_t k, const float *b_dev,
                                  uint64_t ldb, float *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);
int spal_csc_krylov_block_f64(spal_csc_t a, int method, spal_csc_t m, uint64_t k, const double *b, uint64_t ldb,
                              uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);
int spal_csc_krylov_block_f32(spal_csc_t a, int method, spal_csc_t m, uint64_t k, const float *b, uint64_t ldb,
                              uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);
int spal_csc_krylov_block_dev_f64(spal_csc_t a, int method, spal_csc_t m, uint64_t k, const double *b_dev,
                                  uint64_t ldb, double *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);
int spal_csc_krylov_block_dev_f32(spal_csc_t a, int method, spal_csc_t m, uint64_t k, const float *b_dev,
                                  uint64_t ldb, float *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);

/* ---- (A - shift I) x = b on the device: MINRES for symmetric indefinite systems ---------------------------
 * Not in the reference.  CG needs a positive definite matrix; BiCGStab and GMRES take anything but waste symmetry.
 * MINRES (Paige-Saunders) runs a three-term Lanczos recurrence: one product per step, a fixed number of vectors, and
 * a residual estimate that never grows, so reason 1 at maxit still returns the best iterate.  Solves
 * (A - shift I) x = b with A symmetric and M symmetric positive definite; neither is checked, as with CG.  The
 * contract is again a sequential text the device reproduces bit for bit, f32 and f64.
 *
 * All scalars are T.  sg = T(shift) is rounded once; shift is a double.  Every product is rounded before the sum it
 * enters (no FMA); sqrt and / are IEEE, correctly rounded.  dot, T(tol * tol) and M^-1 (two exact solves on m, or
 * "trsv_sweeps" sweeps per triangle, or v itself when m == NULL) are those of the CG / BiCGStab section above.
 *
 *   zb = M^-1 b;  bb = dot(b, zb);  thr = T(tol * tol) * bb
 *   q = A x;  r2[i] = b[i] - (q[i] - (sg * x[i]));  y = M^-1 r2
 *   beta = sqrt(dot(r2, y));  phibar = beta;  pp = phibar * phibar;  it = 0;  test
 *   oldb = dbar = epsln = 0;  cs = -1;  sn = 0;  r1 = w = w2 = 0
 *   s = 1 / beta;  v[i] = y[i] * s
 *   while not stopped:
 *     q = A v;  c1 = (it == 0 ? 0 : beta / oldb)
 *     t[i] = (q[i] - (sg * v[i])) - (c1 * r1[i]);  alfa = dot(v, t)
 *     c2 = alfa / beta;  t[i] = t[i] - (c2 * r2[i]);  r1 = r2;  r2 = t
 *     y = M^-1 r2;  oldb = beta;  beta = sqrt(dot(r2, y));  it += 1
 *     oldeps = epsln;  delta = (cs * dbar) + (sn * alfa);  gbar = (sn * dbar) - (cs * alfa)
 *     epsln = sn * beta;  dbar = -(cs * beta);  gamma = sqrt((gbar * gbar) + (beta * beta))
 *     cs = gbar / gamma;  sn = beta / gamma;  phi = cs * phibar;  phibar = sn * phibar;  denom = 1 / gamma
 *     w1 = w2;  w2 = w;  w[i] = ((v[i] - (oldeps * w1[i])) - (delta * w2[i])) * denom
 *     x[i] = x[i] + (phi * w[i])
 *     pp = phibar * phibar;  test                                   -- x already holds this iteration's update
 *     s = 1 / beta;  v[i] = y[i] * s
 *   test (on pp):  pp <= thr: stop, reason 0;  else pp not finite: stop, reason 2;  else it == maxit: stop, reason 1
 *
 * pp is the recurrence's estimate of ||r||^2 in the M^-1 norm and bb the same norm of b; without m these are ||r||^2
 * and dot(b, b), CG's criterion.  info.residual_sq = pp and info.rhs_sq = bb.
 * No value raises an error: an indefinite M (dot(r2, y) < 0, so sqrt gives NaN), a singular A - shift I (gamma == 0)
 * or an overflow all reach pp as NaN and stop with reason 2.  The lucky breakdown beta == 0 gives sn = 0, so
 * pp = 0 <= thr: the iteration stops with reason 0 before 1 / beta is formed.  There is no max(gamma, eps) clamp and
 * no second set of stopping rules: one test, as everywhere else in the library.
 *
 * spal_*_minres_*: the arguments of spal_*_krylov_* without `method` and with `double shift` after m; the _dev forms
 * SYNCHRONISE `stream` and are refused on a capturing stream.  spal_*_minres_block_*: the arguments of
 * spal_*_krylov_block_* without `method`, with one shift for all columns: k independent iterations in lockstep on
 * shared launches.  Column j and infos[j] are the vector text's bits for B[:, j] (with SpMM's products and the block
 * solves as M^-1, as in the block section above), whatever k, the leading dimensions, "krylov_tile",
 * "krylov_check_every" and the other columns are; a stopped column is frozen, and a NaN in one column never reaches
 * another.  Refusals, status codes, spal_krylov_info, the options read, the plans built before the first iteration
 * and the locks (none held across a product) are those of the CG / BiCGStab entries; additionally a shift that is NaN
 * or infinite is SPAL_ERR_INVALID_ARGUMENT.  The messages begin "spal_csr_minres" / "spal_csr_minres_block" (csc
 * alike).  Work vectors: v, three for r1 / r2 / t, two for w1 / w2 (w is written over w1), y only with m; with m a
 * block call whose ldb > k packs B once.
 * describe()["krylov"] (the block calls: ["krylov_block"]) after a call has "method": "minres" and gains "shift".
 * Not provided: an AMG hierarchy as M, shift-invert eigsh on top of this, MINRES-QLP for singular systems, capture
 * into a graph. */
int spal_csr_minres_f64(spal_csr_t a, spal_csr_t m, double shift, const double *b, uint64_t b_len, double *x,
                        uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_minres_f32(spal_csr_t a, spal_csr_t m, double shift, const float *b, uint64_t b_len, float *x,
                        uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_minres_dev_f64(spal_csr_t a, spal_csr_t m, double shift, const double *b_dev, double *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info);   /* synchronises */
int spal_csr_minres_dev_f32(spal_csr_t a, spal_csr_t m, double shift, const float *b_dev, float *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_minres_f64(spal_csc_t a, spal_csc_t m, double shift, const double *b, uint64_t b_len, double *x,
                        uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_minres_f32(spal_csc_t a, spal_csc_t m, double shift, const float *b, uint64_t b_len, float *x,
                        uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_minres_dev_f64(spal_csc_t a, spal_csc_t m, double shift, const double *b_dev, double *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_minres_dev_f32(spal_csc_t a, spal_csc_t m, double shift, const float *b_dev, float *x_dev, double tol,
                            uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csr_minres_block_f64(spal_csr_t a, spal_csr_t m, double shift, uint64_t k, const double *b, uint64_t ldb,
                              uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);                            /* host blocks; info: k records */
int spal_csr_minres_block_f32(spal_csr_t a, spal_csr_t m, double shift, uint64_t k, const float *b, uint64_t ldb,
                              uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);
int spal_csr_minres_block_dev_f64(spal_csr_t a, spal_csr_t m, double shift, uint64_t k, const double *b_dev,
                                  uint64_t ldb, double *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);                        /* synchronises; info on the host */
int spal_csr_minres_block_dev_f32(spal_csr_t a, spal_csr_t m, double shift, uint64_t k, const float *b_dev,
                                  uint64_t ldb, float *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);
int spal_csc_minres_block_f64(spal_csc_t a, spal_csc_t m, double shift, uint64_t k, const double *b, uint64_t ldb,
                              uint64_t b_rows, double *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);
int spal_csc_minres_block_f32(spal_csc_t a, spal_csc_t m, double shift, uint64_t k, const float *b, uint64_t ldb,
                              uint64_t b_rows, float *x, uint64_t ldx, uint64_t x_rows, double tol, uint64_t maxit,
                              spal_krylov_info *info);
int spal_csc_minres_block_dev_f64(spal_csc_t a, spal_csc_t m, double shift, uint64_t k, const double *b_dev,
                                  uint64_t ldb, double *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);
int spal_csc_minres_block_dev_f32(spal_csc_t a, spal_csc_t m, double shift, uint64_t k, const float *b_dev,
                                  uint64_t ldb, float *x_dev, uint64_t ldx, double tol, uint64_t maxit, void *stream,
                                  spal_krylov_info *info);

/* ---- A x = b on the device: restarted GMRES(m), right-preconditioned ------------------------------------
 * Not in the reference.  For matrices that are not symmetric, where BiCGStab can break down (on the cyclic shift with
 * b = e0 it returns reason 2 after one iteration; GMRES solves that system in n steps).  The contract is again a
 * sequential text the device reproduces bit for bit, f32 and f64.  All scalars are T.  dot, thr = T(tol * tol) * bb,
 * M^-1 (two exact solves on m, or "trsv_sweeps" sweeps per triangle, or v itself when m == NULL) and the stop reasons
 * are exactly those of the section above.  Every product is rounded before the sum or difference it enters (no FMA);
 * sqrt and / are IEEE, correctly rounded.  m = restart.  The basis is orthogonalised by two passes of classical
 * Gram-Schmidt (CGS2); H is the (m + 1) x m Hessenberg matrix after the rotations (cs, sn), g the rotated right-hand side.
 *
 *   bb = dot(b, b);  thr = T(tol * tol) * bb;  it = 0
 *   cycle:
 *     q = A x;  r[i] = b[i] - q[i];  rr = dot(r, r)
 *     test on rr:  rr <= thr: stop 0;  else rr not finite: stop 2;  else it == maxit: stop 1      (residual_sq = rr)
 *     beta = sqrt(rr);  v_0[i] = r[i] / beta;  g[0] = beta;  jj = 0
 *     repeat:
 *       j = jj;  z = M^-1 v_j;  w = A z
 *       h[k] = dot(v_k, w)                      k = 0..j     (all from the same w)
 *       w[i] = (..((w[i] - (h[0]*v_0[i])) - (h[1]*v_1[i])) ..) - (h[j]*v_j[i])
 *       c[k] = dot(v_k, w)                      k = 0..j
 *       w[i] = the same update with c;   h[k] = h[k] + c[k]
 *       hn = sqrt(dot(w, w));  v_{j+1}[i] = w[i] / hn;  it += 1
 *       for k = 0..j-1:  t = (cs[k]*h[k]) + (sn[k]*h[k+1]);  h[k+1] = (cs[k]*h[k+1]) - (sn[k]*h[k]);  h[k] = t     (h[j+1] = hn)
 *       d = sqrt((h[j]*h[j]) + (hn*hn));  cs[j] = h[j]/d;  sn[j] = hn/d;  h[j] = d
 *       g[j+1] = -(sn[j]*g[j]);  g[j] = cs[j]*g[j];  H[0..j, j] = h[0..j];  est = g[j+1]*g[j+1];  jj = j + 1
 *       if est not finite:  stop 2, residual_sq = est, x is what it was at the start of this cycle
 *       until est <= thr or it == maxit or jj == m
 *     back substitution, column form:  for k = jj-1 .. 0:  y[k] = g[k] / H[k,k];  g[l] = g[l] - (H[l,k]*y[k]) for l < k
 *     u[i] = (..((y[0]*v_0[i]) + (y[1]*v_1[i])) ..) + (y[jj-1]*v_{jj-1}[i]);   x[i] = x[i] + (M^-1 u)[i]
 *     goto cycle
 *
 * Consequences.  (1) Reasons 0 and 1 are always decided on the TRUE residual, recomputed at the head of a cycle; est
 * only ends a cycle.  (2) Every cycle performs at least one iteration, so maxit bounds the call.  (3) On a lucky
 * breakdown (hn == 0 with h[j] != 0) v_{j+1} is a vector of NaN: it is written and never read, because sn[j] = 0 gives
 * est = 0 and ends the cycle.  A zero matrix gives cs = 0 / 0: reason 2 at it = 1 with x untouched.
 *
 * On the device one kernel forms the first level of all j + 1 dot products of a pass from one read of w,
 * one workgroup per k finishes them, one kernel applies all j + 1 updates from one read of w (the second one fused with
 * the first level of dot(w, w)), and one workgroup does the step's scalar arithmetic in a block of device memory.
 * "krylov_check_every" on `a` counts INNER iterations between two polls, with the defaults of the section above; the
 * host also polls when its own count reaches restart, and after the head of a cycle that follows an early end.  Every
 * kernel reads the block's flags (written by an earlier launch on the same stream: nothing waits, nothing spins) and
 * returns before it writes once the call has stopped or, for the kernels of a step, once the cycle has ended; x,
 * iterations, reason and residual_sq do not depend on the interval.  "trsv_sweeps" on m works as above.  The basis
 * (restart + 1 vectors), w, q, with m also z and u, and two more vectors for sweeps come from the caching allocator in
 * ONE block per call on 256-byte strides; no handle lock is held across a product or a solve.  The _dev forms
 * SYNCHRONISE `stream` and cannot be captured into a graph.
 * SPAL_ERR_INVALID_ARGUMENT: everything spal_*_krylov_* refuses (there is no method here), and restart == 0 or
 * restart > 256 (one Hessenberg column element per thread of the 256-thread scalar workgroup).
 * SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  SPAL_ERR_OUT_OF_MEMORY: no room for the basis.  Nothing leaks.
 * describe() on `a` gains "gmres" after a call: {restart, preconditioned, precond_sweeps, iterations, cycles, reason,
 * check_every, polls, dot_batch = basis vectors per batch of the two kernels, basis_bytes = that one block, solve_ms};
 * "krylov" is left to CG and BiCGStab.
 * Not provided: capture into a graph, flexible GMRES, several GPUs, a multi-dot fused into the SpMV kernels. */
int spal_csr_gmres_f64(spal_csr_t a, spal_csr_t m, const double *b, uint64_t b_len, double *x, uint64_t x_len,
                       uint64_t restart, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_gmres_f32(spal_csr_t a, spal_csr_t m, const float *b, uint64_t b_len, float *x, uint64_t x_len,
                       uint64_t restart, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_gmres_dev_f64(spal_csr_t a, spal_csr_t m, const double *b_dev, double *x_dev, uint64_t restart,
                           double tol, uint64_t maxit, void *stream, spal_krylov_info *info);   /* synchronises */
int spal_csr_gmres_dev_f32(spal_csr_t a, spal_csr_t m, const float *b_dev, float *x_dev, uint64_t restart,
                           double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_gmres_f64(spal_csc_t a, spal_csc_t m, const double *b, uint64_t b_len, double *x, uint64_t x_len,
                       uint64_t restart, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_gmres_f32(spal_csc_t a, spal_csc_t m, const float *b, uint64_t b_len, float *x, uint64_t x_len,
                       uint64_t restart, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_gmres_dev_f64(spal_csc_t a, spal_csc_t m, const double *b_dev, double *x_dev, uint64_t restart,
                           double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_gmres_dev_f32(spal_csc_t a, spal_csc_t m, const float *b_dev, float *x_dev, uint64_t restart,
                           double tol, uint64_t maxit, void *stream, spal_krylov_info *info);

/* ---- A X = B on the device: restarted GMRES(m) for a block of k right-hand sides --------------------------
 * Not in the reference.  ONE call runs k INDEPENDENT restarted GMRES iterations in lockstep on shared launches: one pass
 * over the matrix per product and one walk of the factor's launches per solve serve all k columns.  It is not block
 * GMRES with a shared Krylov space: every column keeps the sequential text above.
 * LAYOUT.  B and X are n x k, dense and ROW-MAJOR: element (i, j) at [i * ld + j], ld >= k, offsets i * ld 64-bit.  X
 * holds X0 on entry and the result on exit.
 * COLUMN j IS THE GMRES TEXT, as written above, applied to B[:, j] and X[:, j], with its own bb, thr, it, jj, h, c, cs,
 * sn, g, H, y, stop test, reason and residual_sq.  dot is the header's dot on the column.  A v is the value
 * spal_*_spmm_* defines.  M^-1 v is column j of spal_*_trsm_*(lower, unit_diag = 1) followed by spal_*_trsm_*(upper,
 * unit_diag = 0); with m's option "trsv_sweeps" = s >= 0 it is column j of the two spal_*_trsm_sweep_* calls; with
 * m == NULL it is v.  Hence x, iterations, reason, residual_sq and rhs_sq of every column are, bit for bit in f32 and
 * f64, what the text gives for that column -- and, on a handle whose SpMV sums rows in sequence, what spal_*_gmres_*
 * returns for it.  solve_ms is the call's device time, the same in all k records.
 * CYCLES ARE COMMON TO THE BLOCK.  All columns that have not stopped begin a cycle together.  Inside the cycle a
 * column takes inner steps until its own text ends its cycle (est <= thr, it == maxit or jj == restart); after that it
 * idles -- no kernel writes anything of it -- until every column still running has ended its cycle.  Then the back
 * substitution, the update of x and the head of the next cycle run for all of them together.  Idling changes no bit of
 * a column's text.  A column that stops is frozen for the rest of the call; the call ends when all k columns have
 * stopped, and every common cycle advances every running column by at least one iteration, so maxit bounds it.
 * Products and solves keep running on all k columns, into work blocks: the steps spent on idle and frozen columns are
 * wasted and accepted -- the columns are not compacted.
 * WHAT THE BITS DO NOT DEPEND ON: k, ldb, ldx, the column tile, "krylov_check_every", the batch of basis blocks, what
 * the other columns hold.  A NaN, an inf, a breakdown or a lucky breakdown in one column never reaches another; on a
 * lucky breakdown v_{j+1} of that column is NaN and is never read.
 * PADDING.  X[i, k..ldx) is never written and B[i, k..ldb) is never read.  X and B must not overlap.
 * SPAL_ERR_INVALID_ARGUMENT before any device work: everything spal_*_gmres_* refuses, restart == 0 and restart > 256
 * included (info points to k records); k == 0; ldb < k or ldx < k; the host forms: b_rows != nrows or x_rows != nrows;
 * x_dev == b_dev.  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  SPAL_ERR_OUT_OF_MEMORY: no room for the basis
 * (the message names the number of blocks, n, k and the bytes); nothing leaks.  The messages begin
 * "spal_csr_gmres_block:" / "spal_csc_gmres_block:".
 * The _dev forms SYNCHRONISE `stream` (they poll) and are refused on a capturing stream.  Before the first step the
 * call builds what spal_*_gmres_* builds, takes the basis (restart + 1 blocks of n x k), w, q and with m also z and u
 * in ONE block on 256-byte strides with packed leading dimension k -- so the products and solves take v_j and w
 * directly --, the dots' scratch and the k scalar records, and grows the stream's sweep scratch to n x k per buffer:
 * no iteration allocates.  The host polls every "krylov_check_every" inner steps, when its count reaches restart (or
 * the steps that bring the column with the fewest iterations to maxit), and after a head that follows an early end; a
 * poll copies the k heads of the scalar records to pinned memory and decides "all stopped" and "every running column
 * has ended its cycle".  No handle lock is held across a product or a solve.  Order between launches comes from the
 * stream alone -- no flags waited on, no spins, no float atomics, no grid syncs.  CSC handles multiply and solve on
 * their CSR twin.  The host forms copy B and X0 up packed, iterate, and copy the k columns of X back.
 * Options on `a`: "krylov_check_every" and "krylov_tile", with the meaning and defaults they have above.
 * describe() on `a` gains "gmres_block" after a call: {restart, k, preconditioned, precond_sweeps, tile,
 * iterations_min, iterations_max, cycles (common cycles), steps (inner steps the host enqueued: steps * k - the sum of
 * the iterations is the idle and wasted work), converged (columns that ended with reason 0), check_every, polls,
 * dot_batch (basis blocks per batch), basis_bytes, solve_ms}; "gmres" and "krylov_block" stay with their own calls.
 * Not provided: compaction of finished or idle columns, per-column cycles out of step, a shared search space, flexible
 * GMRES, capture into a graph, several GPUs. */
int spal_csr_gmres_block_f64(spal_csr_t a, spal_csr_t m, uint64_t k, const double *b, uint64_t ldb, uint64_t b_rows,
                             double *x, uint64_t ldx, uint64_t x_rows, uint64_t restart, double tol, uint64_t maxit,
                             spal_krylov_info *info);
int spal_csr_gmres_block_f32(spal_csr_t a, spal_csr_t m, uint64_t k, const float *b, uint64_t ldb, uint64_t b_rows,
                             float *x, uint64_t ldx, uint64_t x_rows, uint64_t restart, double tol, uint64_t maxit,
                             spal_krylov_info *info);
int spal_csr_gmres_block_dev_f64(spal_csr_t a, spal_csr_t m, uint64_t k, const double *b_dev, uint64_t ldb,
                                 double *x_dev, uint64_t ldx, uint64_t restart, double tol, uint64_t maxit, void *stream,
                                 spal_krylov_info *info);
int spal_csr_gmres_block_dev_f32(spal_csr_t a, spal_csr_t m, uint64_t k, const float *b_dev, uint64_t ldb,
                                 float *x_dev, uint64_t ldx, uint64_t restart, double tol, uint64_t maxit, void *stream,
                                 spal_krylov_info *info);
int spal_csc_gmres_block_f64(spal_csc_t a, spal_csc_t m, uint64_t k, const double *b, uint64_t ldb, uint64_t b_rows,
                             double *x, uint64_t ldx, uint64_t x_rows, uint64_t restart, double tol, uint64_t maxit,
                             spal_krylov_info *info);
int spal_csc_gmres_block_f32(spal_csc_t a, spal_csc_t m, uint64_t k, const float *b, uint64_t ldb, uint64_t b_rows,
                             float *x, uint64_t ldx, uint64_t x_rows, uint64_t restart, double tol, uint64_t maxit,
                             spal_krylov_info *info);
int spal_csc_gmres_block_dev_f64(spal_csc_t a, spal_csc_t m, uint64_t k, const double *b_dev, uint64_t ldb,
                                 double *x_dev, uint64_t ldx, uint64_t restart, double tol, uint64_t maxit, void *stream,
                                 spal_krylov_info *info);
int spal_csc_gmres_block_dev_f32(spal_csc_t a, spal_csc_t m, uint64_t k, const float *b_dev, uint64_t ldb,
                                 float *x_dev, uint64_t ldx, uint64_t restart, double tol, uint64_t maxit, void *stream,
                                 spal_krylov_info *info);

/* ---- eigsh: the k largest or smallest eigenpairs of a symmetric matrix on the device ----------------------
 * Not in the reference.  Thick-restart Lanczos with full orthogonalisation.  A is taken to be symmetric;
 * as with CG, that is not checked.  The contract is again a sequential text the device reproduces bit for bit, f32 and
 * f64.  The vectors and the scalars of a step are T; the projected problem is solved in double for both element types.
 * dot is the dot above; every product is rounded before the sum or difference it enters (no FMA); sqrt and / are IEEE.
 * m = ncv.  A step is the GMRES step above without the rotations and without M:
 *
 *   step(j):  w = A v_j
 *             h[t] = dot(v_t, w)                     t = 0..j     (all from the same w)
 *             w[i] = (..((w[i] - (h[0]*v_0[i])) - (h[1]*v_1[i])) ..) - (h[j]*v_j[i])
 *             c[t] = dot(v_t, w)                     t = 0..j
 *             w[i] = the same update with c;   h[t] = h[t] + c[t]
 *             hn = sqrt(dot(w, w));  v_{j+1}[i] = w[i] / hn;  products += 1
 *             S[t, j] = S[j, t] = double(h[t])       t = 0..j     (exact conversions; no tridiagonal structure is assumed)
 *
 *   v0 given by the caller, or v0[i] = T((mix32((i + seed) mod 2^32) >> 8) + 1) / T(2^24)  (exact in f32; mix32 is the
 *   colouring's, below);   v_0[i] = v0[i] / sqrt(dot(v0, v0))
 *   S = 0 (m x m doubles);  keep = 0;  restarts = products = 0
 *   phase:
 *     for j = keep .. m-1:  step(j);  jj = j + 1;  if hn is not finite: stop 2;  if hn == 0: leave the loop (exhausted)
 *     if any S[r, q], r, q < jj, is not finite: stop 2
 *     (theta, Y) = jacobi(S[0..jj, 0..jj]), ordered: descending theta for which = LA, ascending for SA, ties by position
 *     res[i] = |double(hn) * Y[jj-1, i]|;   nk = min(k, jj)
 *     converged = the number of leading i < nk with res[i] <= tol * max_t |theta_t|
 *     if exhausted:  stop 0 if jj >= k, else stop 3        (the pairs of the jj x jj problem are final: res = 0)
 *     if converged == k: stop 0;   if restarts == maxit: stop 1
 *     keep = min(k + (m - k) / 2, m - 1)                    (integer division)
 *     new v_c[i] = (..((T(Y[0,c]) * v_0[i]) + (T(Y[1,c]) * v_1[i])) ..) + (T(Y[m-1,c]) * v_{m-1}[i])    c = 0..keep-1
 *     new v_keep = the old v_m;   S = diag(theta_0 .. theta_{keep-1});   restarts += 1;   goto phase
 *   stop 0, 1, 3:  theta[i] = T(theta_i), resid[i] = T(res[i]) for i < nk;  X[:, c] = the sum above over t < jj for c < nk.
 *                  theta[nk..k), resid[nk..k) and X[:, nk..k) are not written (reason 3 alone has nk < k; converged = nk).
 *   stop 2:        theta, resid and X are not written;  converged = 0.
 *
 *   jacobi(S), m x m, on doubles with + - * / sqrt alone:  Y = I;  at most 64 sweeps;  a sweep visits p = 0..m-2,
 *   q = p+1..m-1 in that order:
 *       a = S[p,q];  if a == 0: next
 *       if |S[p,p]| + |a| == |S[p,p]| and |S[q,q]| + |a| == |S[q,q]|:  S[p,q] = S[q,p] = 0;  next
 *       th = (0.5 * (S[q,q] - S[p,p])) / a;  t = 1 / (|th| + sqrt((th*th) + 1));  if th < 0: t = -t
 *       c = 1 / sqrt((t*t) + 1);  s = t * c
 *       S[p,p] = S[p,p] - (t*a);  S[q,q] = S[q,q] + (t*a);  S[p,q] = S[q,p] = 0
 *       for r != p, q:  (x, y) = (S[r,p], S[r,q]);  S[r,p] = S[p,r] = (c*x) - (s*y);  S[r,q] = S[q,r] = (s*x) + (c*y)
 *       for every r:    (x, y) = (Y[r,p], Y[r,q]);  Y[r,p] = (c*x) - (s*y);           Y[r,q] = (s*x) + (c*y)
 *   and stops after the first sweep that rotated nothing.  theta_i = S[i,i], its vector column i of Y.
 *   spal_eigsh_jacobi runs exactly this on the host (s: m x m by rows, symmetric and finite, 1 <= m <= 256; theta: m;
 *   y: m x m by rows; sweeps may be NULL): the pairs are NOT ordered by it.  It is a DIAGNOSTIC AID -- it lets a test or a
 *   binding compare its own restatement of the text with the library's bits without a device -- and no dense
 *   eigensolver to build on: O(m^3) per sweep, one thread.
 *
 * Consequences.  (1) Because every step orthogonalises against the whole basis, the arrow entries S[t, keep], t < keep,
 * of the phase after a restart fall out of the same dots: there is no separate formula for them.  (2) res[i] is the
 * residual norm of pair i in exact arithmetic.  (3) The Ritz vectors are sums of rounded products: their norm is 1 only
 * up to rounding.  (4) MULTIPLE EIGENVALUES: a single-vector Lanczos iteration sees one direction of an eigenspace, so an
 * eigenvalue of multiplicity > 1 is returned ONCE (until rounding brings in a second copy, much later); the pairs
 * returned are then not the k extreme eigenvalues counted with multiplicity.  (5) A start vector orthogonal to a wanted
 * eigenvector misses it the same way; v0 = e_0 on a diagonal matrix exhausts the space at jj = 1.
 * WHAT THE BITS DO NOT DEPEND ON: "krylov_check_every" (unused here: the host polls once per phase), the rotation
 * kernel's form and tiling ("eigsh_rotate"), the batch of basis vectors in the dots and updates, ldx, the stream.
 *
 * On the device the step is GMRES's kernels, the step's scalars (h + c, the column of S, hn, jj and the
 * flags) one workgroup; hn == 0, a hn that is not finite and jj == m are decided there, and every later launch of the
 * phase returns before it writes -- nothing waits, nothing spins.  The host copies the head and the columns of the
 * phase down (one poll per phase), solves the projected problem and decides.  The rotation V <- V Y is one kernel in one
 * of two forms with the same bits.  Option "eigsh_rotate" on `a` (spal_*_set_option): 2 = LDS row tiles: a workgroup stages
 * a tile of rows x m basis values in LDS (about 16 KiB; 64 rows at least, so up to 128 KiB at m = 256 in f64) and emits
 * all keep outputs from it, in place, no second basis; 1 = batched passes, eight outputs per pass over the basis, out of
 * place into a second basis of ncv + 1 vectors; 0 = automatic = 2, the faster of the two in every case measured (n = 1M
 * and 10M, ncv = 30, f32 and f64: DESIGN 3.25); anything else SPAL_ERR_INVALID_ARGUMENT.
 * Arguments: theta and resid are k HOST values in every form; x may be NULL (values only), else it is n x k ROW-MAJOR with
 * leading dimension ldx >= k and X[i, k..ldx) is never written; v0 may be NULL (the default vector from `seed`).
 * The _dev forms take v0_dev and x_dev as device pointers, SYNCHRONISE `stream` and are refused on a capturing stream.
 * The basis (ncv + 1 vectors), w, and with "eigsh_rotate" = 1 a second basis come from the caching allocator in ONE
 * block per call on 256-byte strides.  CSC handles run on their CSR twin.
 * info: restarts, products, converged, reason (0 converged or exhausted with jj >= k, 1 maxit restarts, 2 not finite,
 * 3 exhausted with jj < k), solve_ms = device time from the first to the last launch.
 * SPAL_ERR_INVALID_ARGUMENT before any device work: null a, theta, resid or info; k == 0; ncv <= k; ncv > 256; which
 * outside {0, 1}; tol negative or not finite; ldx < k; an _f64 entry on an f32 handle or the reverse; a matrix that is
 * not square; ncv > nrows; the host forms: v0_len != nrows (with v0), theta_len != k, resid_len != k, x_rows != nrows
 * (with x).  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  SPAL_ERR_OUT_OF_MEMORY: no room for the basis, with the
 * byte count.  Nothing leaks on any failure.
 * describe() on `a` gains "eigsh" after a call: {k, which, ncv, keep, restarts, products, converged, reason, polls,
 * rotate, rotate_tile_rows, basis_bytes, rotate_ms = device time of the restarts' rotations, solve_ms}.
 * Not provided: shift-invert (clustered EXTREME values have the polynomial filter of the next section,
 * spal_*_eigsh_filtered_*, INTERIOR ones the delta filter after it, spal_*_eigsh_near_*), which = LM / BE, nonsymmetric matrices, a generalised problem, block Lanczos,
 * several GPUs, capture into a graph. */
enum { SPAL_EIGSH_LA = 0, SPAL_EIGSH_SA = 1 };
typedef struct spal_eigsh_info {
    uint64_t restarts, products, converged;
    int reason;
    double solve_ms;
} spal_eigsh_info;
int spal_eigsh_jacobi(uint64_t m, const double *s, double *theta, double *y, uint64_t *sweeps);   /* host only */
int spal_csr_eigsh_f64(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const double *v0, uint64_t v0_len,
                       uint64_t seed, double tol, uint64_t maxit, double *theta, uint64_t theta_len, double *resid,
                       uint64_t resid_len, double *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_info *info);
int spal_csr_eigsh_f32(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const float *v0, uint64_t v0_len,
                       uint64_t seed, double tol, uint64_t maxit, float *theta, uint64_t theta_len, float *resid,
                       uint64_t resid_len, float *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_info *info);
int spal_csr_eigsh_dev_f64(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const double *v0_dev, uint64_t seed,
                           double tol, uint64_t maxit, double *theta, double *resid, double *x_dev, uint64_t ldx,
                           void *stream, spal_eigsh_info *info);                  /* synchronises */
int spal_csr_eigsh_dev_f32(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const float *v0_dev, uint64_t seed,
                           double tol, uint64_t maxit, float *theta, float *resid, float *x_dev, uint64_t ldx,
                           void *stream, spal_eigsh_info *info);
int spal_csc_eigsh_f64(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const double *v0, uint64_t v0_len,
                       uint64_t seed, double tol, uint64_t maxit, double *theta, uint64_t theta_len, double *resid,
                       uint64_t resid_len, double *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_info *info);
int spal_csc_eigsh_f32(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const float *v0, uint64_t v0_len,
                       uint64_t seed, double tol, uint64_t maxit, float *theta, uint64_t theta_len, float *resid,
                       uint64_t resid_len, float *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_info *info);
int spal_csc_eigsh_dev_f64(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const double *v0_dev, uint64_t seed,
                           double tol, uint64_t maxit, double *theta, double *resid, double *x_dev, uint64_t ldx,
                           void *stream, spal_eigsh_info *info);
int spal_csc_eigsh_dev_f32(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const float *v0_dev, uint64_t seed,
                           double tol, uint64_t maxit, float *theta, float *resid, float *x_dev, uint64_t ldx,
                           void *stream, spal_eigsh_info *info);

/* ---- the Chebyshev filter: cheb_apply, gershgorin, and eigsh on a polynomial of A ---------------------------
 * Not in the reference.  Where the wanted eigenvalues are clustered, eigsh above spends its time in Gram-Schmidt passes
 * and restarts; Lanczos on p(A), a scaled Chebyshev polynomial that is small on the unwanted part of the spectrum and
 * grows monotonically towards the wanted end, needs 10-30 times fewer of both for about as many products.
 * The contract is again a sequential text the device returns bit for bit, f32 and f64.  Vectors and a step's scalars
 * are T; every product is rounded before the sum or difference it enters (no FMA); dot is the dot above.
 *
 *   THE PRODUCT ORDER IS THE FILTER'S OWN and does not depend on the handle's plan:
 *     rowsum(y, r) = (..((+0.0 + (a[p]*y[col[p]])) + (a[p+1]*y[col[p+1]])) ..)
 *   over the stored entries of row r of the CSR form in storage order; a CSC handle uses its CSR twin (a row's entries
 *   in column order).
 *
 *   coefficients (host doubles; T(.) is the one conversion):
 *     c = (lo+hi)/2;  e = (hi-lo)/2;  s_1 = e/(a0 - c);  s_i = 1/(2/s_1 - s_{i-1})
 *     alpha_1 = T(s_1/e);  beta_1 = 0;   alpha_i = T((2*s_i)/e);  beta_i = T(s_{i-1}*s_i);   cT = T(c)
 *   a0 lies outside [lo, hi]: p(a0) = 1, |s_i| < 1, and nothing overflows in f32 at any degree.
 *
 *   cheb_apply(x; d, lo, hi, a0) = t_d:
 *     t_0 = x
 *     t_1[r] = alpha_1 * (rowsum(t_0, r) - (cT*t_0[r]))
 *     t_i[r] = (alpha_i * (rowsum(t_{i-1}, r) - (cT*t_{i-1}[r]))) - (beta_i*t_{i-2}[r])          i = 2..d
 *
 *   gershgorin(A) = (glo, ghi), in double (f32 values convert exactly): per row r, d = the stored entry (r, r), 0 where
 *   there is none; s = the |off-diagonal entries| added in storage order onto +0.0; glo = min_r (d - s), ghi =
 *   max_r (d + s): enclosures of the spectrum of a symmetric A up to double rounding.  If any row's d - s or d + s is
 *   not finite, both are NaN.
 *
 *   filtered eigsh = the text of eigsh above with five changes (tol == 0 stands for 256 * eps(T) here: a TRUE residual
 *   does not reach eps * scale; the floors the text reaches are in DESIGN 3.26):
 *   1. (glo, ghi) = gershgorin(A); not finite: stop 2 at once.  a0 = ghi for LA, glo for SA; scale = max(|glo|, |ghi|).
 *   2. The interval.  Given [lo, hi]: refused unless lo < hi and a0 lies strictly outside it on the wanted side (a0 > hi
 *      for LA, a0 < lo for SA).  Automatic: the eigsh text above UNCHANGED -- its product is the handle's -- with
 *      maxit = min(warmup, maxit); theta, resid and X are written by it.  A reason other than 1: that result is the
 *      call's (warm_restarts = restarts, warm_products = products; lo = hi = 0).  Else cut = double(theta[k-1]);
 *      unless glo < cut < ghi the warm-up's result is again the call's; else [lo, hi] = [glo, cut] for LA, [cut, ghi]
 *      for SA, and the iteration starts again from the same v0 with restarts = products = 0.
 *   3. In step(j), w = cheb_apply(v_j; d, lo, hi, a0) and products += d.  The pairs (mu, Y) of the projected problem are
 *      ordered DESCENDING for both values of `which`: p is largest at the wanted end.
 *   4. At the end of a phase (after the test of S for values that are not finite), ROTATE FIRST, so that a restart
 *      goes on from the same columns:  kc = min(keep, jj);  x_c[i] = the sum of eigsh's rotation over t < jj, c < kc.
 *      Then for c < nk = min(k, jj):
 *        q_c[r] = rowsum(x_c, r);  products += 1;   th_c = dot(x_c, q_c)
 *        r_c[i] = q_c[i] - (th_c*x_c[i]);           res_c = sqrt(dot(r_c, r_c))
 *      any th_c or res_c not finite: stop 2.  converged = the number of leading c < nk with double(res_c) <= tol * scale.
 *      exhausted (hn == 0, jj <= m): stop 0 if jj >= k, else stop 3 with converged = nk, as in eigsh.
 *      converged == k: stop 0;  restarts == maxit: stop 1;  else new v_c = x_c for c < keep, new v_keep = the old v_m,
 *      S = diag(mu_0 .. mu_{keep-1}), restarts += 1.
 *   5. stop 0, 1, 3:  theta[c] = th_c, resid[c] = res_c, X[:, c] = x_c for c < nk.  stop 2: nothing is written (after an
 *      automatic warm-up theta, resid and X hold the warm-up's values); converged = 0.
 *   th_c is the Rayleigh quotient's numerator: x_c has norm 1 up to rounding (eigsh's consequence 3).
 * WHAT THE BITS DO NOT DEPEND ON: the handle's plan (after the warm-up), the chunk of the step kernel ("cheb_chunk"),
 * "eigsh_rotate", ldx, the stream.
 *
 * On the device (spal_cheb.hip) one recurrence step is one launch of a streaming kernel: a workgroup owns
 * 256 consecutive rows, walks their contiguous entries in chunks, its lanes load values and columns coalesced, gather
 * the vector and write the rounded products to LDS, and each row's thread adds its own products in order, its
 * accumulator carried across chunks -- any row length gives the text's bits.  The d launches are ordered by the stream,
 * the coefficients are kernel arguments, nothing waits and nothing is polled inside a step.  The same kernel without
 * the epilogue gives q_c.  A filtered phase polls twice: the columns of S, then the nk true pairs.  Option
 * "cheb_chunk" on `a`: entries per chunk, 0 = 16 KiB of products (2048 f64, 4096 f32), else 256, 512, 1024, 2048 or 4096.
 *
 * spal_*_cheb_apply_*: x and out are n values (host forms: x_len = out_len = nrows); the _dev forms enqueue `degree`
 * launches on `stream`, take one work vector from the stream's scratch (degree >= 2) and do not synchronise.
 * SPAL_ERR_INVALID_ARGUMENT before any device work: null a, x or out; degree outside 1 .. 256; lo, hi or a0 not finite;
 * lo >= hi; a0 inside [lo, hi]; a dtype mismatch; a matrix that is not square; out overlapping x; wrong lengths.
 * spal_*_gershgorin: square matrices with at least one row; synchronises.
 * spal_*_eigsh_filtered_*: eigsh's arguments plus degree (1 .. 256), automatic (1: lo and hi are ignored; 0: the given
 * interval) and warmup (restarts of the warm-up; the bindings default to 5).  Refused before any device work as eigsh is,
 * and for a degree outside 1 .. 256, automatic outside {0, 1}, a given interval that is not finite or has lo >= hi, a
 * null info; the place of a0 needs Gershgorin's bounds and is refused right after them.  Refused on a capturing stream
 * and on row-block handles as eigsh is.  The recurrence's work vector joins eigsh's one allocation per call.
 * info: eigsh's fields for the filtered iteration (products = d per step + 1 per true residual), or the warm-up's when
 * its result is the call's; warm_restarts, warm_products; lo, hi (0, 0: no filtered phase ran), a0, degree; solve_ms
 * covers both.  describe() on `a` gains "eigsh_filter" after a call: {k, which, ncv, keep, degree, interval, lo, hi,
 * a0, glo, ghi, warm_restarts, warm_products, restarts, products, converged, reason, polls, chunk, basis_bytes,
 * residual_ms, solve_ms}; an automatic call's warm-up also rewrites "eigsh", being an eigsh call.
 * Not provided: shift-invert (interior eigenvalues have the delta filter of the next section), Rayleigh-Ritz on A in
 * the filtered space, automatic choice of the degree, an interval updated between restarts (it breaks the Lanczos
 * relation), Chebyshev as a smoother or preconditioner (cheb_apply is the piece for it), several GPUs, graph capture. */
typedef struct spal_eigsh_filter_info {
    uint64_t restarts, products, converged;
    int reason;
    double solve_ms;
    uint64_t warm_restarts, warm_products;
    double lo, hi, a0;
    uint64_t degree;
} spal_eigsh_filter_info;
int spal_csr_cheb_apply_f64(spal_csr_t a, const double *x, uint64_t x_len, double *out, uint64_t out_len, uint64_t degree,
                            double lo, double hi, double a0);
int spal_csr_cheb_apply_f32(spal_csr_t a, const float *x, uint64_t x_len, float *out, uint64_t out_len, uint64_t degree,
                            double lo, double hi, double a0);
int spal_csr_cheb_apply_dev_f64(spal_csr_t a, const double *x_dev, double *out_dev, uint64_t degree, double lo, double hi,
                                double a0, void *stream);                          /* not synchronised */
int spal_csr_cheb_apply_dev_f32(spal_csr_t a, const float *x_dev, float *out_dev, uint64_t degree, double lo, double hi,
                                double a0, void *stream);
int spal_csc_cheb_apply_f64(spal_csc_t a, const double *x, uint64_t x_len, double *out, uint64_t out_len, uint64_t degree,
                            double lo, double hi, double a0);
int spal_csc_cheb_apply_f32(spal_csc_t a, const float *x, uint64_t x_len, float *out, uint64_t out_len, uint64_t degree,
                            double lo, double hi, double a0);
int spal_csc_cheb_apply_dev_f64(spal_csc_t a, const double *x_dev, double *out_dev, uint64_t degree, double lo, double hi,
                                double a0, void *stream);
int spal_csc_cheb_apply_dev_f32(spal_csc_t a, const float *x_dev, float *out_dev, uint64_t degree, double lo, double hi,
                                double a0, void *stream);
int spal_csr_gershgorin(spal_csr_t a, double *glo, double *ghi);                    /* synchronises */
int spal_csc_gershgorin(spal_csc_t a, double *glo, double *ghi);
int spal_csr_eigsh_filtered_f64(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const double *v0, uint64_t v0_len,
                                uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo,
                                double hi, uint64_t warmup, double *theta, uint64_t theta_len, double *resid,
                                uint64_t resid_len, double *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_filter_info *info);
int spal_csr_eigsh_filtered_f32(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const float *v0, uint64_t v0_len,
                                uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo,
                                double hi, uint64_t warmup, float *theta, uint64_t theta_len, float *resid,
                                uint64_t resid_len, float *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_filter_info *info);
int spal_csr_eigsh_filtered_dev_f64(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const double *v0_dev, uint64_t seed,
                                    double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                    uint64_t warmup, double *theta, double *resid, double *x_dev, uint64_t ldx,
                                    void *stream, spal_eigsh_filter_info *info);   /* synchronises */
int spal_csr_eigsh_filtered_dev_f32(spal_csr_t a, uint64_t k, int which, uint64_t ncv, const float *v0_dev, uint64_t seed,
                                    double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                    uint64_t warmup, float *theta, float *resid, float *x_dev, uint64_t ldx, void *stream,
                                    spal_eigsh_filter_info *info);
int spal_csc_eigsh_filtered_f64(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const double *v0, uint64_t v0_len,
                                uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo,
                                double hi, uint64_t warmup, double *theta, uint64_t theta_len, double *resid,
                                uint64_t resid_len, double *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_filter_info *info);
int spal_csc_eigsh_filtered_f32(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const float *v0, uint64_t v0_len,
                                uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo,
                                double hi, uint64_t warmup, float *theta, uint64_t theta_len, float *resid,
                                uint64_t resid_len, float *x, uint64_t ldx, uint64_t x_rows, spal_eigsh_filter_info *info);
int spal_csc_eigsh_filtered_dev_f64(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const double *v0_dev, uint64_t seed,
                                    double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                    uint64_t warmup, double *theta, double *resid, double *x_dev, uint64_t ldx,
                                    void *stream, spal_eigsh_filter_info *info);
int spal_csc_eigsh_filtered_dev_f32(spal_csc_t a, uint64_t k, int which, uint64_t ncv, const float *v0_dev, uint64_t seed,
                                    double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                    uint64_t warmup, float *theta, float *resid, float *x_dev, uint64_t ldx, void *stream,
                                    spal_eigsh_filter_info *info);

/* ---- the Chebyshev series, the delta filter, and eigsh near sigma --------------------------------------------
 * Not in the reference.  eigsh and its filter above reach the ENDS of the spectrum.  The k eigenvalues nearest a given
 * sigma INSIDE it come from Lanczos on rho(A), rho a damped Chebyshev expansion of a delta function at sigma: the
 * eigenvalues nearest sigma are the largest of rho(A).  Only products with A are needed: there is no shift-invert (the
 * library has no sparse direct solver, and no Krylov solver of it solves a mid-spectrum shifted system: README).  The
 * series sum_i coef_i T_i(A) x this stands on is a call of its own: the building block of matrix functions and spectral
 * densities.  Sequential texts again, returned bit for bit in f32 and f64; T is the handle's type, every product is
 * rounded before the sum or difference it enters (no FMA), rowsum and dot are the ones above.
 *
 *   cheb_series(x; d, lo, hi, coef[0..d]) = s, coef host doubles, T(.) the one conversion:
 *     c = (lo+hi)/2;  e = (hi-lo)/2;  a1 = T(1/e);  a2 = T(2/e);  cT = T(c);  k_i = T(coef[i])
 *     t_0 = x                                                   s[r] = k_0 * t_0[r]
 *     t_1[r] = a1 * (rowsum(t_0, r) - (cT*t_0[r]))              s[r] = s[r] + (k_1 * t_1[r])
 *     t_i[r] = (a2 * (rowsum(t_{i-1}, r) - (cT*t_{i-1}[r]))) - t_{i-2}[r]
 *                                                               s[r] = s[r] + (k_i * t_i[r])     i = 2..d
 *   The T_i are unscaled: |t_i| <= |x| while the spectrum lies in [lo, hi], so nothing overflows in f32.  An eigenvalue
 *   outside the interval makes the t_i grow: the caller's error; it ends in values that are not finite.
 *
 *   cheb_delta_coefficients(d, gamma), -1 < gamma < 1, host doubles, only + - * / (no libm call):
 *     m_0 = 1;  m_1 = gamma;  m_i = ((2*gamma)*m_{i-1}) - m_{i-2}
 *     g_i = double(d+1-i) / double(d+1)                    (Fejer damping: the kernel is nonnegative)
 *     u_i = g_i * m_i   for i = 0,   g_i * (2*m_i)   for i >= 1
 *     nrm = (..((0 + u_0*m_0) + u_1*m_1) .. + u_d*m_d)     (= rho(gamma) before scaling)
 *     coef_i = u_i / nrm
 *   (Jackson damping needs cos(pi*i/(d+2)) and its bits would hang on a libm; the series takes any coefficients.)
 *
 *   eigsh near sigma = the filtered eigsh text above with these changes:
 *   1. (glo, ghi) = gershgorin(A); not finite: stop 2.  scale = max(|glo|, |ghi|).
 *   2. The interval.  Automatic: m = (ghi - glo)/1024, lo = glo - m, hi = ghi + m (an eigenvalue rounding has put a hair
 *      outside Gershgorin's bounds stays inside [-1, 1]).  Given: lo < hi, both finite; the caller vouches that it
 *      encloses the spectrum.  Either way lo < sigma < hi or the call is refused.  gamma = (sigma - c)/e;
 *      coef = cheb_delta_coefficients(d, gamma); nrm zero or not finite: refused.
 *   3. There is no warm-up.
 *   4. In step(j), w = cheb_series(v_j; d, lo, hi, coef) and products += d.  The pairs of the projected problem are
 *      ordered descending.
 *   5. The phase end (rotate first, q_c, th_c, r_c, res_c, converged, the stops, the restart) and the outputs are the
 *      filtered text's.  theta, resid and X so come back in DESCENDING ORDER OF THE FILTER VALUE: inside the main lobe
 *      that is ascending distance from sigma.  The text does not re-sort.
 *   THE TWO-TO-ONE LIMITATION: rho(lambda) = rho(lambda') for two eigenvalues at the same filter value -- exactly so for
 *   a spectrum symmetric about sigma (the 1-D Laplacian at sigma = 2).  rho(A) then has double eigenvalues, single-vector
 *   Lanczos sees one mixed direction per pair, and the call ends with reason 1 and residuals that do not fall.  Move
 *   sigma off the centre of symmetry.  (A block iteration would cure it; a Rayleigh-Ritz step on A would not.)
 * WHAT THE BITS DO NOT DEPEND ON: the handle's plan (no warm-up runs: the plan plays no part at all), "cheb_chunk",
 * "cheb_series_form", "eigsh_rotate", ldx, the stream.
 *
 * On the device (spal_cheb.hip) a series step is ONE launch of the streaming step kernel above with the
 * accumulation in its epilogue: the row's thread holds t_i[r], reads s[r], adds k_i * t_i[r] and writes it back.  Option
 * "cheb_series_form" on `a`: 0 = automatic = 1 = that fused form; 2 = the recurrence step and a separate accumulation
 * launch (the same bits; kept for the measurement in DESIGN 3.28).
 *
 * spal_*_cheb_series_*: x and out are n values (host forms: x_len = out_len = nrows), coef is coef_len = degree + 1 host
 * doubles.  The _dev forms enqueue `degree` launches on `stream`, take two work vectors from the stream's scratch, only
 * read x, and do not synchronise.  SPAL_ERR_INVALID_ARGUMENT before any device work: null a, x, out or coef; degree
 * outside 1 .. 4096; coef_len != degree + 1; lo, hi or a coefficient not finite; lo >= hi; a dtype mismatch; a matrix
 * that is not square; out overlapping x; wrong lengths.  Capturing streams and row-block handles are refused.
 * spal_cheb_delta_coefficients: host only.  Refused: a null coef; degree outside 1 .. 4096; coef_len != degree + 1;
 * gamma not strictly inside (-1, 1); nrm zero or not finite.  coef is written only on success.
 * spal_*_eigsh_near_*: the filtered eigsh's arguments with sigma in place of which, and no warmup.  Refused before any
 * device work as eigsh is, and for a degree outside 2 .. 4096, a sigma that is not finite, automatic outside {0, 1}, a
 * given interval that is not finite, is empty or does not hold sigma strictly inside, a null info; with an automatic
 * interval the place of sigma is refused right after Gershgorin's bounds.  Capturing streams and row-block handles are
 * refused as eigsh refuses them.  info: eigsh's fields (products = d per step + 1 per true residual), lo, hi (0, 0:
 * stop 2 before an interval was there), sigma, gamma, degree.  describe() on `a` gains "eigsh_near" after a call:
 * {k, sigma, gamma, ncv, keep, degree, interval, lo, hi, glo, ghi, restarts, products, converged, reason, polls, chunk,
 * form, basis_bytes, residual_ms, solve_ms}.
 * Not provided: shift-invert, a block or LOBPCG-type iteration (which would cure exact ties), Rayleigh-Ritz on A in the
 * filtered space, automatic choice of the degree, graph capture, several GPUs. */
typedef struct spal_eigsh_near_info {
    uint64_t restarts, products, converged;
    int reason;
    double solve_ms;
    double lo, hi, sigma, gamma;
    uint64_t degree;
} spal_eigsh_near_info;
int spal_cheb_delta_coefficients(uint64_t degree, double gamma, double *coef, uint64_t coef_len);   /* host only */
int spal_csr_cheb_series_f64(spal_csr_t a, const double *x, uint64_t x_len, double *out, uint64_t out_len, uint64_t degree,
                             double lo, double hi, const double *coef, uint64_t coef_len);
int spal_csr_cheb_series_dev_f64(spal_csr_t a, const double *x_dev, double *out_dev, uint64_t degree, double lo, double hi,
                                 const double *coef, uint64_t coef_len, void *stream);   /* not synchronised */
int spal_csr_cheb_series_f32(spal_csr_t a, const float *x, uint64_t x_len, float *out, uint64_t out_len, uint64_t degree,
                             double lo, double hi, const double *coef, uint64_t coef_len);
int spal_csr_cheb_series_dev_f32(spal_csr_t a, const float *x_dev, float *out_dev, uint64_t degree, double lo, double hi,
                                 const double *coef, uint64_t coef_len, void *stream);   /* not synchronised */
int spal_csc_cheb_series_f64(spal_csc_t a, const double *x, uint64_t x_len, double *out, uint64_t out_len, uint64_t degree,
                             double lo, double hi, const double *coef, uint64_t coef_len);
int spal_csc_cheb_series_dev_f64(spal_csc_t a, const double *x_dev, double *out_dev, uint64_t degree, double lo, double hi,
                                 const double *coef, uint64_t coef_len, void *stream);   /* not synchronised */
int spal_csc_cheb_series_f32(spal_csc_t a, const float *x, uint64_t x_len, float *out, uint64_t out_len, uint64_t degree,
                             double lo, double hi, const double *coef, uint64_t coef_len);
int spal_csc_cheb_series_dev_f32(spal_csc_t a, const float *x_dev, float *out_dev, uint64_t degree, double lo, double hi,
                                 const double *coef, uint64_t coef_len, void *stream);   /* not synchronised */
int spal_csr_eigsh_near_f64(spal_csr_t a, uint64_t k, double sigma, uint64_t ncv, const double *v0, uint64_t v0_len,
                            uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                            double *theta, uint64_t theta_len, double *resid, uint64_t resid_len, double *x, uint64_t ldx,
                            uint64_t x_rows, spal_eigsh_near_info *info);
int spal_csr_eigsh_near_dev_f64(spal_csr_t a, uint64_t k, double sigma, uint64_t ncv, const double *v0_dev, uint64_t seed,
                                double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                double *theta, double *resid, double *x_dev, uint64_t ldx, void *stream,
                                spal_eigsh_near_info *info);   /* synchronises */
int spal_csr_eigsh_near_f32(spal_csr_t a, uint64_t k, double sigma, uint64_t ncv, const float *v0, uint64_t v0_len,
                            uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                            float *theta, uint64_t theta_len, float *resid, uint64_t resid_len, float *x, uint64_t ldx,
                            uint64_t x_rows, spal_eigsh_near_info *info);
int spal_csr_eigsh_near_dev_f32(spal_csr_t a, uint64_t k, double sigma, uint64_t ncv, const float *v0_dev, uint64_t seed,
                                double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                float *theta, float *resid, float *x_dev, uint64_t ldx, void *stream,
                                spal_eigsh_near_info *info);   /* synchronises */
int spal_csc_eigsh_near_f64(spal_csc_t a, uint64_t k, double sigma, uint64_t ncv, const double *v0, uint64_t v0_len,
                            uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                            double *theta, uint64_t theta_len, double *resid, uint64_t resid_len, double *x, uint64_t ldx,
                            uint64_t x_rows, spal_eigsh_near_info *info);
int spal_csc_eigsh_near_dev_f64(spal_csc_t a, uint64_t k, double sigma, uint64_t ncv, const double *v0_dev, uint64_t seed,
                                double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                double *theta, double *resid, double *x_dev, uint64_t ldx, void *stream,
                                spal_eigsh_near_info *info);   /* synchronises */
int spal_csc_eigsh_near_f32(spal_csc_t a, uint64_t k, double sigma, uint64_t ncv, const float *v0, uint64_t v0_len,
                            uint64_t seed, double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                            float *theta, uint64_t theta_len, float *resid, uint64_t resid_len, float *x, uint64_t ldx,
                            uint64_t x_rows, spal_eigsh_near_info *info);
int spal_csc_eigsh_near_dev_f32(spal_csc_t a, uint64_t k, double sigma, uint64_t ncv, const float *v0_dev, uint64_t seed,
                                double tol, uint64_t maxit, uint64_t degree, int automatic, double lo, double hi,
                                float *theta, float *resid, float *x_dev, uint64_t ldx, void *stream,
                                spal_eigsh_near_info *info);   /* synchronises */

/* ---- KPM moments: the spectral density and eigenvalue counts ---------------------------------------------------
 * Not in the reference.  The calls above need a degree and a number of wanted pairs; what says whether they are adequate
 * is HOW MANY EIGENVALUES LIE IN AN INTERVAL, and more generally the spectral density.  The kernel polynomial method
 * gives both from products with A alone: the Chebyshev moments mu_i = z^T T_i(A) z of k random probe columns estimate
 * trace(T_i(A)), the damped series of the moments is the density, and its integral over [a, b] the count.  This call
 * returns the moments; the damping, the density and the count are host arithmetic on them (the Python layer's
 * kpm_damping, kpm_density, kpm_count: host doubles with cos, NOT bit-pinned).  A sequential text again, returned bit
 * for bit in f32 and f64; T is the handle's type, every product is rounded before the sum or difference it enters (no
 * FMA); rowsum, dot, mix32 and gershgorin are the ones above.
 *
 *   probes.  Given by the caller (an n x k block, row-major, leading dimension ldz >= k), or hashed:
 *       h(i) = mix32((i + seed) mod 2^32);   z[i, j] = mix32((h(i) + j) mod 2^32) >> 31 ? T(-1) : T(+1)
 *     (Rademacher entries; only seed mod 2^32 enters, as for the colouring.)
 *
 *   interval.  Automatic: gershgorin's with the margin of eigsh-near (m = (ghi-glo)/1024, lo = glo-m, hi = ghi+m),
 *     not finite: refused as there.  Given: lo < hi, finite; the caller vouches that it encloses the spectrum.
 *     c, e, a1 = T(1/e), a2 = T(2/e), cT = T(c) as in cheb_series.
 *
 *   kpm_moments(A; d, Z) for one column z (columns are independent; d >= 1; m = ceil(d/2)):
 *       t_0 = z
 *       t_1[r] = a1 * (rowsum(t_0, r) - (cT*t_0[r]))
 *       t_i[r] = (a2 * (rowsum(t_{i-1}, r) - (cT*t_{i-1}[r]))) - t_{i-2}[r]              i = 2..m
 *       mu_0 = dot(t_0, t_0);   mu_1 = dot(t_1, t_0)
 *       mu_{2i}   = (T(2)*dot(t_i, t_i))     - mu_0      1 <= i,  2i   <= d
 *       mu_{2i+1} = (T(2)*dot(t_{i+1}, t_i)) - mu_1      1 <= i,  2i+1 <= d
 *     out[i*k + j] = double(mu_i of column j)   (exact conversions);   products = m per column.
 *
 *   The doubling identities T_{2i} = 2 T_i^2 - 1 and T_{2i+1} = 2 T_{i+1} T_i - T_1 need a symmetric A (not checked, as
 *   for CG and eigsh); they halve the passes over the matrix.  An eigenvalue outside the interval makes the t_i grow:
 *   the caller's error; it ends in values that are not finite, which are returned as they are.  A NaN or inf in one
 *   column never reaches another column.  A matrix without rows has every moment +0.0 (given interval only).
 * WHAT THE BITS DO NOT DEPEND ON: k, ldz, the other columns' contents, "cheb_chunk", "kpm_tile", "kpm_form", the
 * handle's plan (it plays no part), the stream.
 *
 * On the device (spal_kpm.hip) a step is ONE launch that advances a tile of columns on one pass over the
 * matrix, with the recurrence and the first level of both dots in its epilogue (a workgroup owns whole tiles of 1024
 * rows), and one small launch that walks the dots' upper levels and writes the step's moments into a device table.
 * Option "kpm_tile" on `a`: the column tile, 0 = automatic (the narrowest of 1, 2, 4, 8 that holds k), else 1, 2, 4 or
 * 8; k beyond the tile takes one pass of the matrix per tile.  Option "kpm_form": 0 = automatic = 1 = the fused kernel;
 * 2 = the same block step without the dots, followed by a block dot launch (the same bits; kept for the measurement in
 * DESIGN 3.29).  "cheb_chunk" applies, clipped so that a chunk's products of one tile stay within 32 KiB of LDS.
 *
 * spal_*_kpm_moments_*: z is NULL (hashed probes from seed) or z_rows x ldz values of which the first k of every row
 * are read; mu receives mu_len = (degree + 1) * k doubles.  The _dev forms take z_dev (NULL or device memory, n rows)
 * and a stream, and their work blocks from the stream's scratch (a second identical call takes no new device memory);
 * the host forms take theirs from the caching allocator.  Both enqueue everything, copy the moments back and
 * synchronise ONCE, at the end; nothing is polled.  (With an automatic interval Gershgorin's bounds are read back
 * first, as eigsh near sigma reads them.)  SPAL_ERR_INVALID_ARGUMENT before any device work: a null a, mu or info;
 * degree outside 1 .. 4096; k outside 1 .. 256; mu_len != (degree + 1) * k; ldz < k; z_rows != nrows; automatic outside
 * {0, 1}; a given interval that is not finite or has lo >= hi; a dtype mismatch; a matrix that is not square.
 * Capturing streams and row-block handles are refused as cheb_series refuses them.  Nothing leaks on failure.
 * info: products (per column), lo, hi, glo, ghi (0, 0 when the interval was given), degree, probes, solve_ms (device
 * time of the launches).  describe() on `a` gains "kpm" after a call: {degree, probes, steps, tile, form, chunk, lo,
 * hi, launches, solve_ms}.
 * Not provided: the damping and the density on the device, probes other than +-1 generated on the device, a stochastic
 * error bound in the C ABI (the Python layer's kpm_count reports the spread over the probes), several GPUs. */
typedef struct spal_kpm_info {
    uint64_t products;
    double lo, hi, glo, ghi;
    uint64_t degree, probes;
    double solve_ms;
} spal_kpm_info;
int spal_csr_kpm_moments_f64(spal_csr_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi,
                             const double *z, uint64_t z_rows, uint64_t ldz, double *mu, uint64_t mu_len,
                             spal_kpm_info *info);
int spal_csr_kpm_moments_dev_f64(spal_csr_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo,
                                 double hi, const double *z_dev, uint64_t ldz, double *mu, uint64_t mu_len, void *stream,
                                 spal_kpm_info *info);   /* synchronises */
int spal_csr_kpm_moments_f32(spal_csr_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi,
                             const float *z, uint64_t z_rows, uint64_t ldz, double *mu, uint64_t mu_len,
                             spal_kpm_info *info);
int spal_csr_kpm_moments_dev_f32(spal_csr_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo,
                                 double hi, const float *z_dev, uint64_t ldz, double *mu, uint64_t mu_len, void *stream,
                                 spal_kpm_info *info);   /* synchronises */
int spal_csc_kpm_moments_f64(spal_csc_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi,
                             const double *z, uint64_t z_rows, uint64_t ldz, double *mu, uint64_t mu_len,
                             spal_kpm_info *info);
int spal_csc_kpm_moments_dev_f64(spal_csc_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo,
                                 double hi, const double *z_dev, uint64_t ldz, double *mu, uint64_t mu_len, void *stream,
                                 spal_kpm_info *info);   /* synchronises */
int spal_csc_kpm_moments_f32(spal_csc_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo, double hi,
                             const float *z, uint64_t z_rows, uint64_t ldz, double *mu, uint64_t mu_len,
                             spal_kpm_info *info);
int spal_csc_kpm_moments_dev_f32(spal_csc_t a, uint64_t degree, uint64_t k, uint64_t seed, int automatic, double lo,
                                 double hi, const float *z_dev, uint64_t ldz, double *mu, uint64_t mu_len, void *stream,
                                 spal_kpm_info *info);   /* synchronises */

/* ---- multicolour reordering: greedy colouring and B = P A P^T -------------------------------------------
 * Not in the reference.  An exact triangular solve costs one launch step per level; numbering the rows
 * colour by colour leaves both triangles of P A P^T with at most as many levels as there are colours.
 * The contract is again a sequential text the device reproduces exactly.
 *
 *   Graph.     A is square with n rows; the vertices are the rows.  i ~ j iff i != j and (i, j) or (j, i) is stored.
 *              Values play no part: a stored zero is an edge.
 *   Priority.  key(i) = mix32((i + seed) mod 2^32), in 32-bit arithmetic
 *                  x ^= x >> 16;  x *= 0x7feb352d;  x ^= x >> 15;  x *= 0x846ca68b;  x ^= x >> 16
 *              a bijection of the 32-bit words: keys are distinct for n < 2^32, no tie-break is needed.
 *              mix32(0) = 0, mix32(1) = 1753845952, mix32(2) = 3507691905, mix32(3) = 1408362973.
 *              `seed` is a uint64_t of which only seed mod 2^32 enters the keys: seed 2^32 + 7 colours as seed 7 does
 *              (host and device alike); describe()["ordering"]["seed"] reports the value as it was given.
 *   Colouring. Visit the vertices by DESCENDING key; a vertex takes the smallest colour >= 0 that no neighbour
 *              visited before it has.  ncolours = the largest colour + 1 (0 for n = 0).
 *   Ordering.  perm maps new -> old and lists the rows by (colour, old row) ascending: a stable counting sort.
 *   Symmetric permutation.  B = P A P^T:  B[i'][j'] = A[perm[i']][perm[j']], columns ascending inside a row, the values
 *              A's bits, moved and never recomputed (f32 and f64 bit-identical, NaN payloads included).  B stores
 *              (i', i') exactly where A stores (perm[i'], perm[i']): ILU(0)'s precondition carries over.
 *
 * Host, no device: spal_colour_greedy is the text on uint64 arrays (it builds the transposed adjacency itself),
 * spal_perm_from_colours the ordering.  Both refuse null pointers, a rowptr that does not ascend from 0 and a column
 * >= n (SPAL_ERR_INVALID_ARGUMENT; a colour >= n likewise).
 *
 * Device (spal_colour.hip).  spal_*_colour returns the text's colours by Jones-Plassmann rounds: a row is READY in
 * round r when every neighbour (of A's row or of A^T's row) with a HIGHER key was coloured in a round before r, and
 * then takes the smallest colour absent among those higher-key neighbours; lower-key neighbours are ignored even when
 * coloured.  Every round is one launch over the rows still uncoloured; order between rounds is stream order alone (no
 * flags, no spins, no grid sync); the host polls a device counter of uncoloured rows after a batch of rounds.
 * *rounds = the longest path of descending keys, counted in vertices (at most n; 0 for n = 0).  colour_host may be NULL.
 * spal_*_permute builds B for ANY permutation perm_host[n] (new -> old) as a new, independent handle of a's type: a
 * relabel-and-gather kernel, then two stable transposes put the columns back in order.  spal_*_multicolour runs
 * colour -> order -> permute with only the poll block crossing to the host.  The result keeps perm on the device:
 * spal_*_ordering downloads it (ncolours = 0 for a handle made by spal_*_permute; a handle without an ordering is
 * refused), spal_*_permute_vec_* moves a vector between the orders:
 *   direction 0:  y[i'] = x[perm[i']]   (into the handle's order)      direction 1:  y[perm[i']] = x[i']   (back)
 * The _dev forms are enqueued on `stream` and not synchronised; colour, permute and multicolour synchronise it.
 * SPAL_ERR_INVALID_ARGUMENT: null arguments; a matrix that is not square; perm that is not a permutation of 0 .. n-1
 * (the message names the first offending position) or n != nrows; direction outside {0, 1}; x == y; vectors of the
 * wrong length or element type.  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  Nothing leaks on failure.
 * describe() of a handle with an ordering gains "ordering": {colours, rounds, seed, colour_ms, permute_ms}.
 * Not provided: applying a permuted factor inside spal_*_krylov_* / _gmres_* (solve the permuted system instead:
 * p = multicolour(a), f = ilu0(p), x = from_order(solve(p, to_order(b), f))). */
int spal_colour_greedy(uint64_t n, const uint64_t *rowptr, const uint64_t *colind, uint64_t seed, uint64_t *colour,
                       uint64_t *ncolours);                                       /* host only */
int spal_perm_from_colours(uint64_t n, const uint64_t *colour, uint64_t *perm);  /* host only */
int spal_csr_colour(spal_csr_t a, uint64_t seed, void *stream, uint64_t *colour_host, uint64_t *ncolours,
                    uint64_t *rounds);
int spal_csc_colour(spal_csc_t a, uint64_t seed, void *stream, uint64_t *colour_host, uint64_t *ncolours,
                    uint64_t *rounds);
int spal_csr_permute(spal_csr_t a, const uint64_t *perm_host, uint64_t n, void *stream, spal_csr_t *out);
int spal_csc_permute(spal_csc_t a, const uint64_t *perm_host, uint64_t n, void *stream, spal_csc_t *out);
int spal_csr_multicolour(spal_csr_t a, uint64_t seed, void *stream, spal_csr_t *out, uint64_t *ncolours);
int spal_csc_multicolour(spal_csc_t a, uint64_t seed, void *stream, spal_csc_t *out, uint64_t *ncolours);
int spal_csr_ordering(spal_csr_t a, uint64_t *perm_host, uint64_t *ncolours);
int spal_csc_ordering(spal_csc_t a, uint64_t *perm_host, uint64_t *ncolours);
int spal_csr_permute_vec_f64(spal_csr_t a, const double *x, uint64_t x_len, double *y, uint64_t y_len,
                             int direction);                                      /* host vectors */
int spal_csr_permute_vec_f32(spal_csr_t a, const float *x, uint64_t x_len, float *y, uint64_t y_len, int direction);
int spal_csr_permute_vec_dev_f64(spal_csr_t a, const double *x_dev, double *y_dev, int direction, void *stream);
int spal_csr_permute_vec_dev_f32(spal_csr_t a, const float *x_dev, float *y_dev, int direction, void *stream);
int spal_csc_permute_vec_f64(spal_csc_t a, const double *x, uint64_t x_len, double *y, uint64_t y_len,
                             int direction);
int spal_csc_permute_vec_f32(spal_csc_t a, const float *x, uint64_t x_len, float *y, uint64_t y_len, int direction);
int spal_csc_permute_vec_dev_f64(spal_csc_t a, const double *x_dev, double *y_dev, int direction, void *stream);
int spal_csc_permute_vec_dev_f32(spal_csc_t a, const float *x_dev, float *y_dev, int direction, void *stream);

/* ---- aggregation AMG: a multigrid cycle as the preconditioner of CG and BiCGStab -----------------------
 * Not in the reference.  Unsmoothed aggregation: the coarse operators are built with the colouring's hashed priority
 * and the COO -> CSR assembly, every step of the cycle is SpMV-shaped.  The contract is again a
 * sequential text the device reproduces bit for bit, in f32 and f64; T is the handle's element type.
 *
 *   Graph.      As for the colouring: A is square with n rows; i ~ j iff i != j and (i, j) or (j, i) is stored.  Values
 *               play no part.  deg(i) = the number of distinct such j (an entry stored in both directions counts once).
 *   Priority.   prio(i) = (min(deg(i), 2^31 - 1) << 32) | mix32((i + seed) mod 2^32), a 64-bit integer; mix32 is the
 *               colouring's.  Distinct for n < 2^32.  The degree comes first on purpose: with the key alone, high-key
 *               roots turn into hubs whose leaves stay singleton aggregates level after level and the coarsening stalls.
 *   Roots.      Visit the vertices by DESCENDING priority; a vertex becomes a root iff no neighbour is a root already.
 *               The roots are a maximal independent set: every other vertex has a root among its neighbours.
 *   Aggregates. Roots are numbered by ascending row; agg[i] = the number of i's root, where the root of a vertex that
 *               is not one is its neighbouring root of highest priority.  nagg = the number of roots (0 for n = 0); an
 *               isolated vertex is an aggregate of one.
 *               The path 0-1-...-7 with seed 0: roots {0, 2, 4, 6}, agg = [0,1,1,2,2,2,3,3].  The 3 x 3 five-point grid
 *               with seed 0: agg = [0,2,1,2,2,2,3,2,4], nagg = 5.  A star stored in one direction only: one aggregate.
 *   Coarse matrix.  A_{l+1} = what the COO -> CSR text (below) makes of the triplets (agg[i], agg[j], v) listed in
 *               A_l's storage order, rows ascending, columns ascending: stable order by (row, col), duplicates summed
 *               left to right in insertion order, results equal to zero dropped.
 *   Hierarchy.  A_0 = A.  Level l + 1 is built while ALL of: n_l > coarse_rows;  l + 1 < max_levels;  nagg < n_l;
 *               every row of A_{l+1} stores its diagonal.  Otherwise level l is the coarsest; L = the number of levels.
 *   Cycle.      w_l[i] = T(omega) / d_l[i], d_l[i] the stored (i, i) entry (IEEE division; a stored zero is no error,
 *               it propagates).
 *                 rowsum(A, x, i):  acc = +0.0;  for each stored (i, j, v) in ascending column, diagonal included:
 *                                   acc = acc + (v * x[j])          (the product rounded: no FMA)
 *                 smooth0(l, b):    x[i] = w_l[i] * b[i]
 *                 smooth(l, b, x):  x'[i] = x[i] + (w_l[i] * (b[i] - rowsum(A_l, x, i)))     (every row from the OLD x)
 *               cycle(l, b) -> x:
 *                 x = smooth0(l, b), then s - 1 times smooth;  s = nu for l < L - 1, coarse_sweeps for l = L - 1
 *                 if l == L - 1: return x
 *                 gamma times:
 *                     r[i]  = b[i] - rowsum(A_l, x, i)
 *                     bc[I] = acc = +0.0;  for the members i of aggregate I in ascending i: acc = acc + r[i]
 *                     e     = cycle(l + 1, bc)
 *                     x[i]  = x[i] + (T(alpha) * e[agg[i]])
 *                 nu times smooth
 *                 return x
 *               With L = 1 the cycle is coarse_sweeps damped Jacobi sweeps.  The operator is linear and fixed; for a
 *               symmetric A it is symmetric (equal pre- and post-smoothing, Jacobi; gamma = 2 squares the correction),
 *               so CG may use it.  NaN goes by position.
 *   Krylov.     spal_*_krylov_amg_* are the two loops of spal_*_krylov_* (above), unchanged, with M^-1 v = cycle(0, v).
 *
 * Parameters (spal_amg_default_params: {0, 16, 64, 2, 16, 1, 2.0 / 3.0, 1.0}): gamma 1 = V cycle, 2 = W cycle.  Refused
 * with SPAL_ERR_INVALID_ARGUMENT and a message that names the field: max_levels outside 1 .. 32, nu outside 1 .. 16,
 * coarse_sweeps outside 1 .. 1024, gamma outside {1, 2}, omega or alpha not finite or <= 0.
 *
 * Host, no device: spal_amg_aggregate is the aggregation text on uint64 arrays (it builds the transposed adjacency
 * itself and refuses what spal_colour_greedy refuses).
 *
 * Device (spal_amg.hip).  Setup builds level after level, ordered by the stream alone (no flags, no spins, no grid
 * sync): degrees by a merge of A's and A^T's rows, the roots by rounds (a vertex decides once every higher-priority
 * neighbour has decided, and becomes a non-root as soon as one of them is a root; the host polls a counter of undecided
 * vertices after a batch of rounds, as the colouring does), the join, the numbering by a scan, the member lists by a
 * stable counting sort, the relabelled triplets through the COO assembly on the device, w_l.  Setup synchronises
 * `stream`.  The hierarchy holds its OWN copy of level 0's CSR arrays (of a CSC handle: its CSR twin's) and outlives
 * `a`.  Every work vector of every level is allocated at setup: an apply allocates nothing.
 * spal_amg_apply_* take host vectors; spal_amg_apply_dev_* are enqueued on `stream` and not synchronised (x_dev ==
 * b_dev is refused; a capturing stream is refused in this version).  Applies on one handle serialise on its lock; a
 * call on another stream than the previous call's first makes that stream wait on an event the handle keeps (no host
 * wait).  The smoother is ONE kernel per sweep (matrix + x + b + w read, x' written to a ping-pong vector); rows of any
 * length keep the text's order of additions while the products of a long row are formed by a whole wave.
 * Option "amg_tail_rows" (spal_amg_set_option; default 1024, values above 4096 are clamped to it, 0 = off): all
 * levels from the first with n_l <= amg_tail_rows down to the coarsest run as ONE single-workgroup launch per visit of
 * that level, with workgroup barriers between the steps.  The bits do not depend on it.
 * spal_amg_describe: {dtype, levels, rows[], nnz[], aggregates[], rounds[], setup_ms[], stopped_by ("coarse_rows",
 * "max_levels", "no_coarsening" or "diagonal"), tail_rows, tail_from_level (= levels when no level runs in the tail),
 * applies, params}.  spal_amg_level_csr returns an independent handle holding A_level; spal_amg_aggregates the agg[]
 * of a level that has a coarser one (len = its rows).
 * spal_*_krylov_amg_*: the arguments of spal_*_krylov_* with `g` where `m` stands; g is not NULL and matches `a` in
 * rows, device and element type (it need not come from `a` itself).  Default "krylov_check_every" is 1, as with a
 * factor; describe()["krylov"] of such a call additionally carries "precond": "amg".
 * SPAL_ERR_INVALID_ARGUMENT: null arguments, wrong lengths, an _f64 entry on an f32 handle or the reverse, a matrix
 * that is not square, a level-0 row without a stored diagonal (the message names the first such row), a level out of
 * range.  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  Nothing leaks on failure.
 * Not provided: smoothed aggregation, a strength-of-connection threshold, K-cycles, graph capture of the cycle, AMG
 * inside spal_*_gmres_* and the block solvers, several GPUs, changing cycle parameters after setup, re-setup on new
 * values with the old aggregates. */
typedef struct spal_amg_params {
    uint64_t seed, max_levels, coarse_rows, nu, coarse_sweeps, gamma;
    double omega, alpha;
} spal_amg_params;
int spal_amg_default_params(spal_amg_params *params);
int spal_amg_aggregate(uint64_t n, const uint64_t *rowptr, const uint64_t *colind, uint64_t seed, uint64_t *agg,
                       uint64_t *nagg);                                           /* host only */
int spal_csr_amg_setup(spal_csr_t a, const spal_amg_params *params, void *stream, spal_amg_t *out);
int spal_csc_amg_setup(spal_csc_t a, const spal_amg_params *params, void *stream, spal_amg_t *out);
int spal_amg_destroy(spal_amg_t g);                                               /* NULL is fine */
int spal_amg_describe(spal_amg_t g, char *buf, size_t buf_len);
int spal_amg_set_option(spal_amg_t g, const char *key, int64_t value);
int spal_amg_level_csr(spal_amg_t g, uint64_t level, spal_csr_t *copy);
int spal_amg_aggregates(spal_amg_t g, uint64_t level, uint64_t *agg_host, uint64_t len);
int spal_amg_apply_f64(spal_amg_t g, const double *b, uint64_t b_len, double *x, uint64_t x_len);
int spal_amg_apply_f32(spal_amg_t g, const float *b, uint64_t b_len, float *x, uint64_t x_len);
int spal_amg_apply_dev_f64(spal_amg_t g, const double *b_dev, double *x_dev, void *stream);
int spal_amg_apply_dev_f32(spal_amg_t g, const float *b_dev, float *x_dev, void *stream);
int spal_csr_krylov_amg_f64(spal_csr_t a, int method, spal_amg_t g, const double *b, uint64_t b_len, double *x,
                            uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_krylov_amg_f32(spal_csr_t a, int method, spal_amg_t g, const float *b, uint64_t b_len, float *x,
                            uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_krylov_amg_dev_f64(spal_csr_t a, int method, spal_amg_t g, const double *b_dev, double *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csr_krylov_amg_dev_f32(spal_csr_t a, int method, spal_amg_t g, const float *b_dev, float *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_krylov_amg_f64(spal_csc_t a, int method, spal_amg_t g, const double *b, uint64_t b_len, double *x,
                            uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_krylov_amg_f32(spal_csc_t a, int method, spal_amg_t g, const float *b, uint64_t b_len, float *x,
                            uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_krylov_amg_dev_f64(spal_csc_t a, int method, spal_amg_t g, const double *b_dev, double *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_krylov_amg_dev_f32(spal_csc_t a, int method, spal_amg_t g, const float *b_dev, float *x_dev, double tol,
                                uint64_t maxit, void *stream, spal_krylov_info *info);

/* ---- FSAI: a factorised sparse approximate inverse, applied by two SpMVs ---------------------------------
 * Not in the reference.  G ~ L^-1 on a prescribed lower-triangular pattern (Kolotilina - Yeremin), M^-1 = Gt * G: every
 * row of G comes from one small dense SPD system, independent of every other row.  The contract is again
 * a sequential text the device reproduces bit for bit, in f32 and f64; T is the handle's element type.
 *
 * fsai(A, S; cap) for a square handle A and a pattern S of the same kind, shape, device and element type (NULL: A
 * itself); S's values are never read.  Only entries on or below the diagonal of A and of S are read: symmetry is
 * assumed, not checked, as with CG.  Every row of S must store its diagonal.  Every product is rounded before the sum
 * or difference it enters (no FMA); sqrt and / are the correctly rounded ones.
 *
 *   structure of G = the entries (i, j), j <= i, of S, in S's storage order (columns ascending)
 *   row i:  Q = the columns of row i of G;  P = the last min(|Q|, cap) of them (so P ends in i);  m = |P|
 *           G[i, j] = +0.0 for j in Q \ P                        (stored zeros: the structure does not depend on cap)
 *           B[s, t] = the stored entry (P[s], P[t]) of A for s >= t, +0.0 where there is none
 *           for j = 0..m-1:                                       (Cholesky by columns, B = C Ct)
 *               d = B[j,j];  for k = 0..j-1:  d = d - (C[j,k]*C[j,k])
 *               if not (d > 0 and d finite):  REJECT row i
 *               C[j,j] = sqrt(d)
 *               for r = j+1..m-1:  t = B[r,j];  for k = 0..j-1:  t = t - (C[r,k]*C[j,k]);   C[r,j] = t / C[j,j]
 *           g[m-1] = 1 / C[m-1,m-1]                               (Ct g = e_m)
 *           for t = m-2 down to 0:  s = +0.0;  for u = t+1..m-1:  s = s + (C[u,t]*g[u]);   g[t] = (0 - s) / C[t,t]
 *           if any g[t] is not finite:  REJECT row i
 *           G[i, P[t]] = g[t]
 *   REJECT row i:  G[i, j] = +0.0 for j != i;  G[i,i] = 1/sqrt(a_ii) if a_ii > 0 and finite and 1/sqrt(a_ii) finite,
 *           else 1;  rejected += 1                                (a_ii = B[m-1,m-1]: the stored (i, i) of A, or +0.0)
 *   Gt = the transpose of G as a CSR matrix (values moved bit for bit)
 *   apply(v) = Gt * (G * v), two products of the handles G and Gt
 *
 * Every element of C has one fixed order of operations.  Consequences: for SPD A no row is rejected, G A Gt has unit
 * diagonal up to rounding, and Gt G is SPD.  Rejection makes the result a well-defined, still SPD, locally Jacobi
 * preconditioner instead of a source of NaN.  THE BITS OF G DO NOT DEPEND ON the stream, which kernel form a row took,
 * a's plan, or CSR or CSC (a CSC handle runs on its CSR twin, as eigsh does).  apply's bits are those of the two
 * handles' own spmv: they equal the sequential row sums of the text wherever the handle's SpMV sums rows in sequence,
 * which is what the solvers say about a's products too.
 * cap is the option "fsai_max_row" on `a` (spal_*_set_option): default 32, valid 1 .. 64, anything else
 * SPAL_ERR_INVALID_ARGUMENT.  It is read when setup is called.
 *
 * Host, no device: spal_fsai_row_* run the text's Cholesky and back-substitution (and its rejected row) on ONE local
 * system, b_lower = B's lower triangle packed by rows (m (m + 1) / 2 values, 1 <= m <= 64), g = m values, *rejected =
 * 0 or 1: a diagnostic aid of the kind of spal_eigsh_jacobi.
 *
 * Device (spal_fsai.hip).  Setup is ordered by the stream alone (no flags, no spins): the counts of S's entries with
 * column <= row, a scan, G's columns, the factor kernel in two forms chosen per row by m (a thread per row with the
 * triangle in registers for m <= thread_form_max; one wave per row with the triangle packed in LDS above it; the
 * rows of the second form are listed by the structure pass), the existing device transpose for Gt, and the plans of
 * both factors, so the first application pays nothing.  Setup synchronises `stream`; f holds its own matrices and
 * outlives `a`.  spal_fsai_apply_* take host vectors; spal_fsai_apply_dev_* are enqueued on `stream` and not
 * synchronised (x_dev == b_dev is refused): two products and nothing else, u = G b in the stream's own scratch block,
 * so, like every call that takes that block, they are refused on a capturing stream.  No lock of f is held across a
 * product; concurrent applies and solves on one f share nothing but its two matrices.
 * spal_fsai_describe: {dtype, rows, nnz, cap, max_row (the largest m), capped_rows, rejected, rows_thread_form,
 * rows_wave_form, block_rows, thread_form_max, setup_ms, structure_ms, kernel_ms, transpose_ms, plan_ms}.
 * spal_fsai_factor_csr returns an independent handle holding G (transposed = 0) or Gt (1).
 * spal_*_krylov_fsai_* / spal_*_minres_fsai_*: the arguments of spal_*_krylov_* / spal_*_minres_* with `f` where `m`
 * stands; f is not NULL and matches `a` in rows, device and element type.  u is one more work vector of the call.
 * describe()["krylov"] of such a call additionally carries "precond": "fsai".
 * SPAL_ERR_INVALID_ARGUMENT: a null `a` or `out`, a matrix that is not square, a pattern of another shape, device or
 * element type, a pattern row without a stored diagonal (the message names the first such row), an _f64 entry on an
 * f32 handle or the reverse, wrong lengths, x_dev == b_dev.  SPAL_ERR_UNSUPPORTED: a handle held as row blocks.  Every
 * refusal is made before or without leaving anything allocated.
 * Not provided: FSAI inside spal_*_gmres_* and the block solvers, adaptive patterns and dropping, a second factor for
 * nonsymmetric A, several GPUs, graph capture of setup. */
int spal_csr_fsai_setup(spal_csr_t a, spal_csr_t pattern /* NULL: a */, void *stream, spal_fsai_t *out);
int spal_csc_fsai_setup(spal_csc_t a, spal_csc_t pattern /* NULL: a */, void *stream, spal_fsai_t *out);
int spal_fsai_destroy(spal_fsai_t f);                                             /* NULL is fine */
int spal_fsai_describe(spal_fsai_t f, char *buf, size_t buf_len);
int spal_fsai_factor_csr(spal_fsai_t f, int transposed, spal_csr_t *copy);
int spal_fsai_apply_f64(spal_fsai_t f, const double *b, uint64_t b_len, double *x, uint64_t x_len);
int spal_fsai_apply_f32(spal_fsai_t f, const float *b, uint64_t b_len, float *x, uint64_t x_len);
int spal_fsai_apply_dev_f64(spal_fsai_t f, const double *b_dev, double *x_dev, void *stream);
int spal_fsai_apply_dev_f32(spal_fsai_t f, const float *b_dev, float *x_dev, void *stream);
int spal_fsai_row_f64(uint64_t m, const double *b_lower, double *g, int *rejected);   /* host only */
int spal_fsai_row_f32(uint64_t m, const float *b_lower, float *g, int *rejected);     /* host only */
int spal_csr_krylov_fsai_f64(spal_csr_t a, int method, spal_fsai_t f, const double *b, uint64_t b_len, double *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_krylov_fsai_f32(spal_csr_t a, int method, spal_fsai_t f, const float *b, uint64_t b_len, float *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_krylov_fsai_dev_f64(spal_csr_t a, int method, spal_fsai_t f, const double *b_dev, double *x_dev, double tol,
                                 uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csr_krylov_fsai_dev_f32(spal_csr_t a, int method, spal_fsai_t f, const float *b_dev, float *x_dev, double tol,
                                 uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_krylov_fsai_f64(spal_csc_t a, int method, spal_fsai_t f, const double *b, uint64_t b_len, double *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_krylov_fsai_f32(spal_csc_t a, int method, spal_fsai_t f, const float *b, uint64_t b_len, float *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_krylov_fsai_dev_f64(spal_csc_t a, int method, spal_fsai_t f, const double *b_dev, double *x_dev, double tol,
                                 uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_krylov_fsai_dev_f32(spal_csc_t a, int method, spal_fsai_t f, const float *b_dev, float *x_dev, double tol,
                                 uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csr_minres_fsai_f64(spal_csr_t a, spal_fsai_t f, double shift, const double *b, uint64_t b_len, double *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_minres_fsai_f32(spal_csr_t a, spal_fsai_t f, double shift, const float *b, uint64_t b_len, float *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csr_minres_fsai_dev_f64(spal_csr_t a, spal_fsai_t f, double shift, const double *b_dev, double *x_dev,
                                 double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csr_minres_fsai_dev_f32(spal_csr_t a, spal_fsai_t f, double shift, const float *b_dev, float *x_dev,
                                 double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_minres_fsai_f64(spal_csc_t a, spal_fsai_t f, double shift, const double *b, uint64_t b_len, double *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_minres_fsai_f32(spal_csc_t a, spal_fsai_t f, double shift, const float *b, uint64_t b_len, float *x,
                             uint64_t x_len, double tol, uint64_t maxit, spal_krylov_info *info);
int spal_csc_minres_fsai_dev_f64(spal_csc_t a, spal_fsai_t f, double shift, const double *b_dev, double *x_dev,
                                 double tol, uint64_t maxit, void *stream, spal_krylov_info *info);
int spal_csc_minres_fsai_dev_f32(spal_csc_t a, spal_fsai_t f, double shift, const float *b_dev, float *x_dev,
                                 double tol, uint64_t maxit, void *stream, spal_krylov_info *info);

/* ---- CSR <-> CSC on the device ------------------------------------------------
 * Replace `impl From<&CscMatrix<T>> for CsrMatrix<T>` (src/csr/conv/csc.rs:4-52)
 * and `impl From<&CsrMatrix<T>> for CscMatrix<T>` (src/csc/conv/csr.rs:4-52),
 * i.e. the counting sort of CsrMatrix::transpose (src/csr.rs:358-406): a stable
 * sort of the entries by their minor index.  Entries are only moved, so the
 * result equals the reference's exactly.  The input handle is unchanged; the
 * output is a new, independent handle. */
int spal_csc_to_csr(spal_csc_t a, spal_csr_t *out);
int spal_csr_to_csc(spal_csr_t a, spal_csc_t *out);

/* ---- C = A * B, sparse x sparse, on the device ----------------------------------
 * Row-wise Gustavson (LDS hash tables per row, expand-sort-compress for rows with more products than the LDS holds).
 * Structure: every (i, j) reached by some k with A[i,k] and B[k,j] stored, sums that are exactly 0.0 KEPT (the
 * reference's Mul drops nothing), columns ascending in every row.  Arithmetic: the products of one (i, j) combined in
 * ascending k, the first one assigned (-x * 0.0 gives -0.0), each rounded before the add (no FMA); f32 in f32.
 * Deterministic: no float atomics.  Options on the LEFT operand (spal_csr_set_option / spal_csc_set_option):
 * "spgemm_route" 0 = auto, 1 = LDS tiers wherever they fit, 2 = every row through the large-row tier; "spgemm_lds_cap"
 * 0 = default, else the largest per-row product count sent to the LDS tiers (at most 4096).  Row-block operands (more than
 * 2^32 - 65537 entries) and products whose nnz or large-row product count passes that limit: SPAL_ERR_UNSUPPORTED.
 * The result plans eagerly; spal_csr_describe / spal_csc_describe on it add a "spgemm" object (rows per tier, products,
 * nnz, route, plan_ms = the result's plan, call_ms). */
/* C = A * B: `impl Mul for &CsrMatrix<T>` (src/csr/ops/mul.rs:5-59), bit-identical. Enqueued on `stream`
 * (NULL = default), synchronised on it (the output size is data dependent). A.ncols must equal B.nrows
 * (assert_eq!, mul.rs:9), same device, same element size. Returns a new, independent handle. */
int spal_csr_mul(spal_csr_t a, spal_csr_t b, void *stream, spal_csr_t *out);
/* `impl Mul for &CscMatrix<T>` (src/csc/ops/mul.rs:5-60). */
int spal_csc_mul(spal_csc_t a, spal_csc_t b, void *stream, spal_csc_t *out);

/* ---- C = A + B, C = A - B, C = -A, on the device ----------------------------------
 * A merge of the two operands' entry streams, cut into equal tiles of the merged sequence.  A and B are both
 * CSR or both CSC, of one shape, device and element type (for CSC read "column" for "row" below).
 * Structure: row i of C holds the union of the columns stored in row i of A and of B, ascending; sums that are exactly
 * zero are KEPT (A - A stores +0.0 at every position of A); nothing is dropped, nothing added.
 * Values: one IEEE operation in the operand type (f32 in f32) -- stored in A only: `a` (bits copied); in B only: `b` for
 * Add, `-b` for Sub (the sign bit flipped: a B-only +0.0 gives -0.0, sub.rs:47); in both: `a + b` / `a - b`.  Equal to
 * the reference bit for bit for finite inputs (subnormals included, no flush to zero) and infinities; a NaN produced by
 * the arithmetic sits at the reference's position, its payload is not part of the contract.  Neg flips the sign bit of
 * every value (+-0, +-inf and NaN included) and copies the structure.
 * Shapes: the reference's CSR and CSC Add / Sub label their transposed intermediate with the untransposed dimensions
 * (SURVEY F9): for nrows > ncols their final transpose indexes out of bounds, for nrows < ncols entries in columns at or
 * beyond nrows are lost and the result is labelled ncols x nrows.  These calls return the union above for every shape.
 * Checks, in the reference's order: null arguments; assert_eq!(nrows, rhs.nrows) then ncols (add.rs:9-10, sub.rs:9-10)
 * -> SPAL_ERR_INVALID_ARGUMENT "assertion failed: nrows == rhs.nrows (left: .., right: ..)"; different devices or element
 * sizes -> SPAL_ERR_INVALID_ARGUMENT; a row-block operand (more than 2^32 - 65537 entries) or a result with more entries
 * than that -> SPAL_ERR_UNSUPPORTED.  Nothing leaks on failure.
 * Calls: enqueued on `stream` (NULL = default) and synchronised on it once (the size of C is data dependent); the
 * operands are only read (several threads may use them at once); each call returns a new, independent handle, planned
 * eagerly.  Option on the LEFT operand (spal_csr_set_option / spal_csc_set_option): "spadd_tile" 0 = default (2048), else
 * a power of two in [16, 2048], the merged elements of one workgroup.  spal_csr_describe / spal_csc_describe on the
 * result add a "spadd" object (op, tile, tiles, matched pairs, nnz, kernel_ms = device time of the kernels, plan_ms =
 * the result's plan, call_ms). */
int spal_csr_add(spal_csr_t a, spal_csr_t b, void *stream, spal_csr_t *out);  /* src/csr/ops/add.rs:5-75 */
int spal_csr_sub(spal_csr_t a, spal_csr_t b, void *stream, spal_csr_t *out);  /* src/csr/ops/sub.rs:5-75 */
int spal_csr_neg(spal_csr_t a, void *stream, spal_csr_t *out);                /* src/csr/ops/neg.rs:5-17 */
int spal_csc_add(spal_csc_t a, spal_csc_t b, void *stream, spal_csc_t *out);  /* src/csc/ops/add.rs:5-70 */
int spal_csc_sub(spal_csc_t a, spal_csc_t b, void *stream, spal_csc_t *out);  /* src/csc/ops/sub.rs:5-70 */
int spal_csc_neg(spal_csc_t a, void *stream, spal_csc_t *out);                /* src/csc/ops/neg.rs:5-17 */

/* ---- COO -> CSR assembly on the device -------------------------------------
 * Replaces `impl From<&CooMatrix<T>> for CsrMatrix<T>`
 * (src/csr/conv/coo.rs:4-115): stable order by (row, col), duplicates summed
 * left to right in insertion order, results equal to zero dropped.
 * Triplets are passed as three arrays (Rust does not fix the layout of
 * Vec<(usize, usize, T)>, so a binding unzips `coo.iter()`, src/coo.rs:491). */
int spal_coo_upload_f64(int device, uint64_t nrows, uint64_t ncols, uint64_t len,
                        const uint64_t *rows, const uint64_t *cols,
                        const double *vals, spal_coo_t *out);
int spal_coo_upload_f32(int device, uint64_t nrows, uint64_t ncols, uint64_t len,
                        const uint64_t *rows, const uint64_t *cols,
                        const float *vals, spal_coo_t *out);
int spal_coo_destroy(spal_coo_t c);
/* Device-resident assembly (the timed path): enqueues on `stream`, returns a
 * new CSR handle.  Synchronises the stream once (the output size is data
 * dependent). */
int spal_coo_assemble_csr(spal_coo_t c, void *stream, spal_csr_t *out);
/* The handle spal_coo_assemble_csr / spal_coo_to_csr_* return is the complete matrix `CsrMatrix::from(&coo)` produces
 * (shape, download, conversions); the plan of the PRODUCT kernels on it (tile heights, x windows, 16-bit columns: ~0.3 ms
 * of small kernels and host round trips at 50M entries) is built by whatever needs it first -- the first product,
 * spal_csr_set_option, spal_csr_autotune_*, spal_csr_alloc_vectors, spal_csr_describe -- or, explicitly, here.  A first
 * product cannot be captured into a graph: plan before capturing.  No-op on handles created from host arrays (planned at
 * create time).  SPAL_COO_EAGER_PLAN=1 plans inside the assembly call as rounds 1-3 did. */
int spal_csr_plan(spal_csr_t a);
/* Same assembly compressed by columns: replaces
 * `impl From<&CooMatrix<T>> for CscMatrix<T>` (src/csc/conv/coo.rs:4-115). */
int spal_coo_assemble_csc(spal_coo_t c, void *stream, spal_csc_t *out);
/* JSON description of the handle and of the route its last assembly took
 * ("local_sort" with its tile geometry, or "general"); for logs and tests. */
int spal_coo_describe(spal_coo_t c, char *buf, size_t buf_len);
/* One-call convenience: upload + assemble + free the COO copy. */
int spal_coo_to_csr_f64(int device, uint64_t nrows, uint64_t ncols, uint64_t len,
                        const uint64_t *rows, const uint64_t *cols,
                        const double *vals, spal_csr_t *out);
int spal_coo_to_csr_f32(int device, uint64_t nrows, uint64_t ncols, uint64_t len,
                        const uint64_t *rows, const uint64_t *cols,
                        const float *vals, spal_csr_t *out);

int spal_coo_to_csc_f64(int device, uint64_t nrows, uint64_t ncols, uint64_t len,
                        const uint64_t *rows, const uint64_t *cols,
                        const double *vals, spal_csc_t *out);
int spal_coo_to_csc_f32(int device, uint64_t nrows, uint64_t ncols, uint64_t len,
                        const uint64_t *rows, const uint64_t *cols,
                        const float *vals, spal_csc_t *out);

/* ---- row-partitioned y = A * x over the GPUs of one node, from one process ---
 * (SURVEY.md sections 8e, 8f-4).  Rows are cut into contiguous ranges with
 * balanced stored entries; every GPU holds its range and a full-length x buffer of
 * which it reads only its WINDOW, the columns its rows store.  The product of a
 * range is the same kernel as the single-GPU path, so results are identical.
 * Exchange steps (RCCL over xGMI, loaded lazily; ngpus == 1 needs no RCCL):
 *   x: spal_mg_csr_broadcast_x (ncclBroadcast of all of x from GPU 0) or
 *      spal_mg_csr_scatter_x (grouped ncclSend/ncclRecv: every GPU receives its
 *      window only);
 *   y: spal_mg_csr_gather_y (slices back to back into GPU 0's y, unequal sizes) or
 *      spal_mg_csr_spmv_resident (kernels + ncclAllGather: all of y on every GPU);
 *   iterative use: spal_mg_csr_spmv_halo (per step every GPU receives only the
 *      entries of y its rows read as columns).
 * devices == NULL means GPUs 0 .. ngpus-1.  transport: 0 = RCCL, 1 = peer copies
 * (hipMemcpyPeerAsync ordered by events; also accepts a device list with repeats,
 * i.e. several shards on one GPU), -1 = RCCL unless the list has repeats. */
int spal_mg_create(int ngpus, const int *devices, spal_mg_t *out);
int spal_mg_create_transport(int ngpus, const int *devices, int transport, spal_mg_t *out);
int spal_mg_destroy(spal_mg_t ctx);
int spal_mg_device_count(spal_mg_t ctx, int *ngpus);
int spal_mg_transport(spal_mg_t ctx, int *transport);
int spal_mg_csr_create_f64(spal_mg_t ctx, uint64_t nrows, uint64_t ncols,
                           const uint64_t *rowptr, uint64_t rowptr_len,
                           const uint64_t *colind, uint64_t colind_len,
                           const double *values, uint64_t values_len,
                           spal_mg_csr_t *out);
int spal_mg_csr_create_f32(spal_mg_t ctx, uint64_t nrows, uint64_t ncols,
                           const uint64_t *rowptr, uint64_t rowptr_len,
                           const uint64_t *colind, uint64_t colind_len,
                           const float *values, uint64_t values_len,
                           spal_mg_csr_t *out);
int spal_mg_csr_destroy(spal_mg_csr_t a);
/* the row boundaries in use: ngpus + 1 entries */
int spal_mg_csr_partition(spal_mg_csr_t a, uint64_t *bounds);
/* per GPU (ngpus entries each): its rows store columns in [need_lo, need_hi) only */
int spal_mg_csr_windows(spal_mg_csr_t a, uint64_t *need_lo, uint64_t *need_hi);
/* bytes one scatter_x / gather_y / halo exchange moves between GPUs (any may be NULL) */
int spal_mg_csr_exchange_bytes(spal_mg_csr_t a, uint64_t *x_scatter, uint64_t *y_gather,
                               uint64_t *halo);
/* host vectors: H2D x to GPU 0, x windows scattered (broadcast when the windows
 * cover most of x), local kernels, y gathered on GPU 0, D2H y */
int spal_mg_csr_spmv_f64(spal_mg_csr_t a, const double *x, uint64_t x_len,
                         double *y, uint64_t y_len);
int spal_mg_csr_spmv_f32(spal_mg_csr_t a, const float *x, uint64_t x_len,
                         float *y, uint64_t y_len);
/* resident (timed) path, everything asynchronous on the context's per-GPU
 * streams until spal_mg_csr_synchronize:
 *   write x into GPU 0's buffer (x_root; the pointer changes with every
 *   spmv_halo), then broadcast_x or scatter_x once;
 *   spmv_local any number of times (kernels only), gather_y: GPU 0's y (nrows
 *   elements, y_gathered) holds the result;
 *   or spmv_resident (kernels + all-gather): GPU 0's copy is at y_root as
 *   ngpus slices of slice_stride elements (slice g holds rows bounds[g] ..);
 *   or, square matrices, spmv_halo any number of times (x <- A * x with the halo
 *   exchange), then gather_y. */
int spal_mg_csr_x_root(spal_mg_csr_t a, void **x_dev);
int spal_mg_csr_broadcast_x(spal_mg_csr_t a);
int spal_mg_csr_scatter_x(spal_mg_csr_t a);
int spal_mg_csr_spmv_local(spal_mg_csr_t a);
int spal_mg_csr_gather_y(spal_mg_csr_t a);
int spal_mg_csr_y_gathered(spal_mg_csr_t a, void **y_dev);
int spal_mg_csr_spmv_halo(spal_mg_csr_t a);
int spal_mg_csr_spmv_resident(spal_mg_csr_t a);
int spal_mg_csr_y_root(spal_mg_csr_t a, void **y_dev, uint64_t *slice_stride);
int spal_mg_csr_synchronize(spal_mg_csr_t a);
/* HIP-event durations (ms, the longest over the GPUs) of the LAST x distribution
 * (broadcast_x / scatter_x), local kernels, halo exchange and y collection
 * (gather_y / the all-gather): ms[0..3]; -1 for a phase that has not run.
 * Synchronises. */
int spal_mg_csr_timing(spal_mg_csr_t a, double *ms);

/* ---- device memory helpers for callers without a HIP binding of their own
 * (the Rust shim, ctypes tests, the C++ tools). ---------------------------- */
int spal_dev_malloc(int device, size_t bytes, void **ptr);
int spal_dev_free(int device, void *ptr);
int spal_memcpy_h2d(int device, void *dst_dev, const void *src_host, size_t bytes);
int spal_memcpy_d2h(int device, void *dst_host, const void *src_dev, size_t bytes);
int spal_device_synchronize(int device);
/* Device blocks released by *_destroy / spal_dev_free are kept in a per-process
 * cache for reuse (bounded by the environment variable SPAL_CACHE_BYTES; default:
 * a quarter of the device's memory, at most half of what was free at first use).
 * spal_cache_trim hands every cached block back to the driver, e.g. before
 * another allocator in the process (torch) needs the memory -- and the placement
 * blocks of spal_csr_alloc_vectors that no live handle holds a piece of, and the
 * per-stream scratch blocks of the sweeps and spal_dot_dev_* (every device that
 * holds some is synchronised first; SPAL_ERR_HIP when a block cannot be returned,
 * for instance while another thread captures a graph). */
int spal_cache_trim(void);

#ifdef __cplusplus
}
#endif
#endif /* SPAL_H */

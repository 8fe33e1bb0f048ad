//! Owned device handles.  A handle is created ONCE per matrix (validation, index narrowing, upload, kernel
//! plan: 0.3 s for 140M entries) and reused for every product; `Drop` releases the device copy.  The host
//! matrix is only borrowed for the duration of `new` (the C ABI copies what it needs).
use std::marker::PhantomData;
use std::os::raw::{c_int, c_void};

use super::{ffi, scalar::{HipKrylov, HipScalar, HipSpmm, HipTrsv}};
use crate::{CooMatrix, CscMatrix, CsrMatrix};

/// `CsrMatrix<T>` resident on a GPU (include/spal.h: spal_csr_t).
pub struct DeviceCsr<T: HipScalar> {
    pub(crate) h: *mut ffi::spal_csr,
    _t: PhantomData<T>,
}
/// `CscMatrix<T>` resident on a GPU (spal_csc_t).
pub struct DeviceCsc<T: HipScalar> {
    pub(crate) h: *mut ffi::spal_csc,
    _t: PhantomData<T>,
}
/// `CooMatrix<T>` triplets resident on a GPU (spal_coo_t): the input of the timed assembly path.
pub struct DeviceCoo<T: HipScalar> {
    pub(crate) h: *mut ffi::spal_coo,
    _t: PhantomData<T>,
}

// The C ABI serialises what needs it (per-handle mutex) and `spmv_dev` is read-only on the handle: a handle
// may move between threads and be shared, like the `Vec`-backed reference types (auto Send + Sync).
unsafe impl<T: HipScalar> Send for DeviceCsr<T> {}
unsafe impl<T: HipScalar> Sync for DeviceCsr<T> {}
unsafe impl<T: HipScalar> Send for DeviceCsc<T> {}
unsafe impl<T: HipScalar> Sync for DeviceCsc<T> {}
unsafe impl<T: HipScalar> Send for DeviceCoo<T> {}

impl<T: HipScalar> Drop for DeviceCsr<T> {
    fn drop(&mut self) { unsafe { ffi::spal_csr_destroy(self.h); } }
}
impl<T: HipScalar> Drop for DeviceCsc<T> {
    fn drop(&mut self) { unsafe { ffi::spal_csc_destroy(self.h); } }
}
impl<T: HipScalar> Drop for DeviceCoo<T> {
    fn drop(&mut self) { unsafe { ffi::spal_coo_destroy(self.h); } }
}

impl<T: HipScalar> DeviceCsr<T> {
    /// Uploads `a` to GPU `device`.  Re-checks the invariants of `CsrMatrix::new` (src/csr.rs:144-156): a
    /// matrix built through the public API passes.
    pub fn new(a: &CsrMatrix<T>, device: i32) -> Self {
        let mut h = std::ptr::null_mut();
        unsafe {
            ffi::check(T::csr_create(device as c_int, a.nrows() as u64, a.ncols() as u64, a.rowptr(), a.colind(),
                                     a.values(), &mut h));
        }
        DeviceCsr { h, _t: PhantomData }
    }
    pub(crate) fn from_raw(h: *mut ffi::spal_csr) -> Self { DeviceCsr { h, _t: PhantomData } }

    /// (nrows, ncols, nnz)  (src/csr.rs:200-222, :287-289)
    pub fn shape(&self) -> (usize, usize, usize) {
        let (mut nr, mut nc, mut nz, mut es) = (0u64, 0u64, 0u64, 0 as c_int);
        unsafe { ffi::check(ffi::spal_csr_shape(self.h, &mut nr, &mut nc, &mut nz, &mut es)); }
        (nr as usize, nc as usize, nz as usize)
    }

    /// y = A * x with host vectors (H2D x, kernel, D2H y).  Panics when `x.len() != ncols`, like
    /// `assert_eq!(self.ncols(), rhs.nrows())` in src/csr/ops/mul.rs:9.
    pub fn mul_vec(&self, x: &[T]) -> Vec<T> {
        let (nrows, ncols, _) = self.shape();
        assert_eq!(ncols, x.len());
        let mut y = vec![T::zero(); nrows];
        unsafe { ffi::check(T::csr_spmv(self.h, x, &mut y)); }
        y
    }

    /// The timed path: `x_dev` (ncols) and `y_dev` (nrows) are device pointers on this handle's GPU, the launch is
    /// enqueued on `stream` (a hipStream_t; null = the default stream) and not synchronised.
    ///
    /// # Safety
    /// the pointers must be valid device allocations of those lengths that do not overlap.
    pub unsafe fn mul_dev(&self, x_dev: *const T, y_dev: *mut T, stream: *mut c_void) {
        ffi::check(T::csr_spmv_dev(self.h, x_dev, y_dev, stream));
    }

    /// Y = A * X for a dense ROW-MAJOR block of `k` vectors (`x.len() == ncols * k`, element (i, j) at `i * k + j`):
    /// one pass over the matrix for all k columns, bit for bit `&A * &X` with every entry of X stored.  Panics like
    /// `assert_eq!(self.ncols(), rhs.nrows())` (src/csr/ops/mul.rs:9) when X has another number of rows.  With one or
    /// two vectors `mul_vec` is the faster call.
    pub fn spmm(&self, x: &[T], k: usize) -> Vec<T> where T: HipSpmm {
        let (nrows, ncols, _) = self.shape();
        assert!(k > 0 && x.len() % k == 0, "X must hold whole rows of k values");
        assert_eq!(ncols, x.len() / k);
        let mut y = vec![T::zero(); nrows * k];
        unsafe { ffi::check(T::csr_spmm(self.h, k as u64, x, k as u64, ncols as u64, &mut y, k as u64, nrows as u64)); }
        y
    }

    /// `spmm` on device pointers with leading dimensions, enqueued on `stream` and not synchronised.
    ///
    /// # Safety
    /// `x_dev` must hold `(ncols - 1) * ldx + k` and `y_dev` `(nrows - 1) * ldy + k` elements; they must not overlap.
    pub unsafe fn spmm_dev(&self, k: usize, x_dev: *const T, ldx: usize, y_dev: *mut T, ldy: usize, stream: *mut c_void)
    where T: HipSpmm {
        ffi::check(T::csr_spmm_dev(self.h, k as u64, x_dev, ldx as u64, y_dev, ldy as u64, stream));
    }

    /// x with L x = b (`lower`) or U x = b for the chosen triangle of this square matrix; entries of the other triangle
    /// are ignored, `unit_diagonal` takes the diagonal as ones.  Bit for bit the sequential substitution of
    /// include/spal.h.  Panics when the matrix is not square, `b.len() != nrows`, or (without `unit_diagonal`) a row
    /// stores no diagonal entry.
    pub fn solve_triangular(&self, b: &[T], lower: bool, unit_diagonal: bool) -> Vec<T> where T: HipTrsv {
        let (nrows, _, _) = self.shape();
        assert_eq!(nrows, b.len());
        let mut x = vec![T::zero(); nrows];
        unsafe { ffi::check(T::csr_trsv(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, b, &mut x)); }
        x
    }

    /// x with A x = b by CG (`ffi::SPAL_KRYLOV_CG`: A symmetric positive definite) or BiCGStab, optionally preconditioned by
    /// `m = self.ilu0(..)`; `x` holds x0 on entry and the result on exit.  Bit for bit the loops of include/spal.h; a
    /// breakdown is no panic but `reason == 2`.  Panics when the matrix is not square or a length differs.
    /// `m.set_option("trsv_sweeps", s)` with s >= 0 makes the call apply `m` by s Jacobi sweeps per triangle instead of
    /// the two exact solves (`self` as `m` with s = 0: Jacobi).
    pub fn solve(&self, method: c_int, m: Option<&DeviceCsr<T>>, b: &[T], x: &mut [T], tol: f64, maxit: u64) -> ffi::spal_krylov_info
    where T: HipKrylov {
        let mut info = ffi::spal_krylov_info::default();
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csr_krylov(self.h, method, mh, b, x, tol, maxit, &mut info)); }
        info
    }

    /// X with A X = B for a row-major block of `k` right-hand sides (`b` and `x` hold nrows * k elements, element (i, j)
    /// at i * k + j; `x` holds X0 on entry): k independent CG / BiCGStab iterations in lockstep on shared launches
    /// (spal_csr_krylov_block_*).  Column j and record j are bit for bit `solve`'s loop on column j, whatever k and the
    /// other columns are; a column that has stopped is frozen while the others run on.  Panics as `solve` does, and when
    /// k == 0 or a block is not nrows x k.
    pub fn solve_block(&self, method: c_int, m: Option<&DeviceCsr<T>>, k: usize, b: &[T], x: &mut [T], tol: f64, maxit: u64)
        -> Vec<ffi::spal_krylov_info>
    where T: HipKrylov {
        assert!(k > 0 && b.len() % k == 0 && x.len() == b.len());
        let mut info = vec![ffi::spal_krylov_info::default(); k];
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csr_krylov_block(self.h, method, mh, k as u64, b, x, tol, maxit, info.as_mut_ptr())); }
        info
    }

    /// x with A x = b by restarted GMRES(`restart`, 1 ..= 256), right-preconditioned by `m` as `solve` is; for matrices
    /// that are not symmetric.  Bit for bit the text of include/spal.h; reasons 0 and 1 are decided on the true residual.
    pub fn gmres(&self, m: Option<&DeviceCsr<T>>, b: &[T], x: &mut [T], restart: u64, tol: f64, maxit: u64) -> ffi::spal_krylov_info
    where T: HipKrylov {
        let mut info = ffi::spal_krylov_info::default();
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csr_gmres(self.h, mh, b, x, restart, tol, maxit, &mut info)); }
        info
    }

    /// X with A X = B for a row-major block of `k` right-hand sides by restarted GMRES(`restart`): k independent
    /// iterations in lockstep on shared launches, with cycles common to the block (spal_csr_gmres_block_*).  `b` and `x`
    /// hold nrows * k elements, element (i, j) at i * k + j; `x` holds X0 on entry.  Column j and record j are bit for
    /// bit `gmres`'s text on column j, whatever k and the other columns are.  Panics as `gmres` does, and when k == 0 or a
    /// block is not nrows x k.
    pub fn gmres_block(&self, m: Option<&DeviceCsr<T>>, k: usize, b: &[T], x: &mut [T], restart: u64, tol: f64, maxit: u64)
        -> Vec<ffi::spal_krylov_info>
    where T: HipKrylov {
        assert!(k > 0 && b.len() % k == 0 && x.len() == b.len());
        let mut info = vec![ffi::spal_krylov_info::default(); k];
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csr_gmres_block(self.h, mh, k as u64, b, x, restart, tol, maxit, info.as_mut_ptr())); }
        info
    }

    /// `solve_triangular` on device pointers (`x_dev == b_dev` solves in place), enqueued on `stream` and not
    /// synchronised once the triangle has its plan (`trsv_analyse`, or the first solve, builds it).
    ///
    /// # Safety
    /// `b_dev` and `x_dev` must hold `nrows` elements each.
    pub unsafe fn solve_triangular_dev(&self, lower: bool, unit_diagonal: bool, b_dev: *const T, x_dev: *mut T, stream: *mut c_void)
    where T: HipTrsv {
        ffi::check(T::csr_trsv_dev(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, b_dev, x_dev, stream));
    }

    /// `sweeps` Jacobi passes `x <- D^-1 (b - N x)` on the chosen triangle instead of the substitution: an approximate
    /// solve whose every pass is one launch of independent rows.  Bit for bit the sequential text of include/spal.h;
    /// from `sweeps = levels - 1` on it is `solve_triangular`'s result.  No host analysis.  Panics as `solve_triangular`.
    pub fn solve_triangular_sweeps(&self, b: &[T], lower: bool, unit_diagonal: bool, sweeps: u64) -> Vec<T> where T: HipTrsv {
        let (nrows, _, _) = self.shape();
        assert_eq!(nrows, b.len());
        let mut x = vec![T::zero(); nrows];
        unsafe { ffi::check(T::csr_trsv_sweep(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, sweeps, b, &mut x)); }
        x
    }

    /// `solve_triangular_sweeps` on device pointers (`x_dev == b_dev` is allowed), enqueued on `stream` and not
    /// synchronised once the handle is prepared (the first sweep call prepares it); scratch comes and goes in stream order.
    ///
    /// # Safety
    /// `b_dev` and `x_dev` must hold `nrows` elements each.
    pub unsafe fn solve_triangular_sweeps_dev(&self, lower: bool, unit_diagonal: bool, sweeps: u64, b_dev: *const T, x_dev: *mut T,
                                              stream: *mut c_void)
    where T: HipTrsv {
        ffi::check(T::csr_trsv_sweep_dev(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, sweeps, b_dev, x_dev, stream));
    }

    /// Builds the solve plan of one triangle now (host level analysis; synchronises `stream`).
    pub fn trsv_analyse(&self, lower: bool, unit_diagonal: bool, stream: *mut c_void) {
        unsafe { ffi::check(ffi::spal_csr_trsv_analyse(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, stream)); }
    }

    /// Setup-time autotune on the caller's device vectors (kernel form, placement of the values array).
    ///
    /// # Safety
    /// as `mul_dev`.
    pub unsafe fn autotune(&self, x_dev: *const T, y_dev: *mut T, stream: *mut c_void, iters: i32) {
        ffi::check(T::csr_autotune(self.h, x_dev, y_dev, stream, iters as c_int));
    }

    /// Device vectors `(x, y)` of `ncols` / `nrows` elements owned by this handle, placed so that the stores of y do
    /// not collide with the matrix stream (include/spal.h: spal_csr_alloc_vectors; a second call returns the same
    /// pointers; freed with the handle).  Setup time: a walk over the device's memory.
    pub fn vectors(&self, stream: *mut c_void) -> (*mut T, *mut T) {
        let (mut x, mut y): (*mut c_void, *mut c_void) = (std::ptr::null_mut(), std::ptr::null_mut());
        unsafe { ffi::check(ffi::spal_csr_alloc_vectors(self.h, &mut x, &mut y, stream)); }
        (x as *mut T, y as *mut T)
    }

    /// Builds the product kernels' plan of a device-assembled handle now (include/spal.h: spal_csr_plan); otherwise its first
    /// product, `set_option`, `autotune` or `vectors` does.  No-op on handles created from host arrays.
    pub fn plan(&self) {
        unsafe { ffi::check(ffi::spal_csr_plan(self.h)); }
    }

    /// Kernel plan knob (include/spal.h: spal_csr_set_option).
    pub fn set_option(&self, key: &str, value: i64) {
        let k = std::ffi::CString::new(key).expect("option key");
        unsafe { ffi::check(ffi::spal_csr_set_option(self.h, k.as_ptr(), value)); }
    }

    /// The device matrix back on the host.  The device upholds `CsrMatrix::new`'s invariants by construction.
    pub fn download(&self) -> CsrMatrix<T> {
        let (nr, nc, nz) = self.shape();
        let (mut rowptr, mut colind, mut values) = (vec![0usize; nr + 1], vec![0usize; nz], vec![T::zero(); nz]);
        unsafe { ffi::check(T::csr_download(self.h, &mut rowptr, &mut colind, &mut values)); }
        CsrMatrix::new(nr, nc, rowptr, colind, values)
    }

    /// Device twin of `impl From<&CsrMatrix<T>> for CscMatrix<T>` (src/csc/conv/csr.rs:4-52): a stable sort of the
    /// entries by column; entries are only moved, so the result equals the reference's exactly.
    pub fn to_csc(&self) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_to_csc(self.h, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }

    /// Device twin of `impl Mul for &CsrMatrix<T>` (src/csr/ops/mul.rs:5-59), bit-identical; synchronises `stream`
    /// (null = the default stream).  Panics when `self.ncols() != rhs.nrows()` (mul.rs:9).
    pub fn mul_mat(&self, rhs: &DeviceCsr<T>, stream: *mut c_void) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_mul(self.h, rhs.h, stream, &mut out)); }
        DeviceCsr::from_raw(out)
    }

    /// Device twins of `impl Add / Sub / Neg for &CsrMatrix<T>` (src/csr/ops/{add,sub,neg}.rs), bit-identical;
    /// synchronise `stream`.  Panic when the shapes differ (add.rs:9-10, sub.rs:9-10).
    pub fn add_mat(&self, rhs: &DeviceCsr<T>, stream: *mut c_void) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_add(self.h, rhs.h, stream, &mut out)); }
        DeviceCsr::from_raw(out)
    }
    pub fn sub_mat(&self, rhs: &DeviceCsr<T>, stream: *mut c_void) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_sub(self.h, rhs.h, stream, &mut out)); }
        DeviceCsr::from_raw(out)
    }
    pub fn neg_mat(&self, stream: *mut c_void) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_neg(self.h, stream, &mut out)); }
        DeviceCsr::from_raw(out)
    }

    /// The ILU(0) factor of this square matrix (spal_csr_ilu0): the same structure, L strictly below the diagonal
    /// (unit diagonal implied), U on and above it, bit for bit the sequential loop without fill; synchronises
    /// `stream`.  `M^-1 r` is `f.trsv(&f.trsv(r, true, true), false, false)`.  The result already has its lower solve
    /// plan.  Panics when the matrix is not square or a row stores no diagonal entry.
    pub fn ilu0(&self, stream: *mut c_void) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_ilu0(self.h, stream, &mut out)); }
        DeviceCsr::from_raw(out)
    }

    /// The greedy colouring of the graph of A + A^T by hashed priority (include/spal.h): exactly the
    /// sequential text, by Jones-Plassmann rounds on the device.  Returns `(colours, ncolours, rounds)`.
    pub fn colour(&self, seed: u64, stream: *mut c_void) -> (Vec<usize>, usize, usize) {
        let (nrows, _, _) = self.shape();
        let mut colours = vec![0u64; nrows];
        let (mut nc, mut rounds) = (0u64, 0u64);
        unsafe { ffi::check(ffi::spal_csr_colour(self.h, seed, stream, colours.as_mut_ptr(), &mut nc, &mut rounds)); }
        (colours.into_iter().map(|c| c as usize).collect(), nc as usize, rounds as usize)
    }

    /// `B = P A P^T`, `B[i'][j'] = A[perm[i']][perm[j']]`, for any permutation `perm` (new -> old); values are moved.
    /// The result keeps `perm` (`ordering`, `permute_vec_dev`).  Panics when `perm` is no permutation of `0..nrows`.
    pub fn permute(&self, perm: &[usize], stream: *mut c_void) -> DeviceCsr<T> {
        let p: Vec<u64> = perm.iter().map(|&i| i as u64).collect();
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csr_permute(self.h, p.as_ptr(), p.len() as u64, stream, &mut out)); }
        DeviceCsr::from_raw(out)
    }

    /// colour -> order by (colour, row) -> permute on the device: both triangles of the result, and of its `ilu0`,
    /// have at most `ordering().1` levels.
    pub fn multicolour(&self, seed: u64, stream: *mut c_void) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        let mut nc = 0u64;
        unsafe { ffi::check(ffi::spal_csr_multicolour(self.h, seed, stream, &mut out, &mut nc)); }
        DeviceCsr::from_raw(out)
    }

    /// `(perm, ncolours)` of a handle made by `permute` (`ncolours == 0`) or `multicolour`; panics on any other handle.
    pub fn ordering(&self) -> (Vec<usize>, usize) {
        let (nrows, _, _) = self.shape();
        let mut perm = vec![0u64; nrows];
        let mut nc = 0u64;
        unsafe { ffi::check(ffi::spal_csr_ordering(self.h, perm.as_mut_ptr(), &mut nc)); }
        (perm.into_iter().map(|i| i as usize).collect(), nc as usize)
    }

    /// `y[i'] = x[perm[i']]` (into this handle's order), or with `back` `y[perm[i']] = x[i']`; enqueued on `stream`.
    ///
    /// # Safety
    /// `x_dev` and `y_dev` must hold `nrows` elements each and must not be the same vector.
    pub unsafe fn permute_vec_dev(&self, x_dev: *const T, y_dev: *mut T, back: bool, stream: *mut c_void) {
        if std::mem::size_of::<T>() == 8 {
            ffi::check(ffi::spal_csr_permute_vec_dev_f64(self.h, x_dev as *const f64, y_dev as *mut f64, back as c_int, stream));
        } else {
            ffi::check(ffi::spal_csr_permute_vec_dev_f32(self.h, x_dev as *const f32, y_dev as *mut f32, back as c_int, stream));
        }
    }
}

impl<T: HipScalar> DeviceCsc<T> {
    pub fn new(a: &CscMatrix<T>, device: i32) -> Self {
        let mut h = std::ptr::null_mut();
        unsafe {
            ffi::check(T::csc_create(device as c_int, a.nrows() as u64, a.ncols() as u64, a.colptr(), a.rowind(),
                                     a.values(), &mut h));
        }
        DeviceCsc { h, _t: PhantomData }
    }

    pub fn shape(&self) -> (usize, usize, usize) {
        let (mut nr, mut nc, mut nz, mut es) = (0u64, 0u64, 0u64, 0 as c_int);
        unsafe { ffi::check(ffi::spal_csc_shape(self.h, &mut nr, &mut nc, &mut nz, &mut es)); }
        (nr as usize, nc as usize, nz as usize)
    }

    /// Device-pointer products of this handle whose neighbour hand-off hit its spin bound (their y was not valid):
    /// include/spal.h: spal_csc_status; call after synchronising the stream.  0 on every other route.
    pub fn invalid_products(&self) -> i32 {
        let mut n: c_int = 0;
        unsafe { ffi::check(ffi::spal_csc_status(self.h, &mut n)); }
        n as i32
    }

    pub fn mul_vec(&self, x: &[T]) -> Vec<T> {
        let (nrows, ncols, _) = self.shape();
        assert_eq!(ncols, x.len());   // src/csc/ops/mul.rs:9
        let mut y = vec![T::zero(); nrows];
        unsafe { ffi::check(T::csc_spmv(self.h, x, &mut y)); }
        y
    }

    /// # Safety
    /// as `DeviceCsr::mul_dev`.
    pub unsafe fn mul_dev(&self, x_dev: *const T, y_dev: *mut T, stream: *mut c_void) {
        ffi::check(T::csc_spmv_dev(self.h, x_dev, y_dev, stream));
    }

    /// As `DeviceCsr::spmm`; runs on the handle's CSR twin whatever "kernel" says, hence the same bits.
    pub fn spmm(&self, x: &[T], k: usize) -> Vec<T> where T: HipSpmm {
        let (nrows, ncols, _) = self.shape();
        assert!(k > 0 && x.len() % k == 0, "X must hold whole rows of k values");
        assert_eq!(ncols, x.len() / k);   // src/csc/ops/mul.rs:9
        let mut y = vec![T::zero(); nrows * k];
        unsafe { ffi::check(T::csc_spmm(self.h, k as u64, x, k as u64, ncols as u64, &mut y, k as u64, nrows as u64)); }
        y
    }

    /// # Safety
    /// as `DeviceCsr::spmm_dev`.
    pub unsafe fn spmm_dev(&self, k: usize, x_dev: *const T, ldx: usize, y_dev: *mut T, ldy: usize, stream: *mut c_void)
    where T: HipSpmm {
        ffi::check(T::csc_spmm_dev(self.h, k as u64, x_dev, ldx as u64, y_dev, ldy as u64, stream));
    }

    /// x with L x = b (`lower`) or U x = b for the chosen triangle of this square matrix; entries of the other triangle
    /// are ignored, `unit_diagonal` takes the diagonal as ones.  Bit for bit the sequential substitution of
    /// include/spal.h.  Runs on the handle's CSR twin.  Panics when the matrix is not square, `b.len() != nrows`, or (without `unit_diagonal`) a row
    /// stores no diagonal entry.
    pub fn solve_triangular(&self, b: &[T], lower: bool, unit_diagonal: bool) -> Vec<T> where T: HipTrsv {
        let (nrows, _, _) = self.shape();
        assert_eq!(nrows, b.len());
        let mut x = vec![T::zero(); nrows];
        unsafe { ffi::check(T::csc_trsv(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, b, &mut x)); }
        x
    }

    /// x with A x = b by CG (`ffi::SPAL_KRYLOV_CG`: A symmetric positive definite) or BiCGStab, optionally preconditioned by
    /// `m = self.ilu0(..)`; `x` holds x0 on entry and the result on exit.  Bit for bit the loops of include/spal.h; a
    /// breakdown is no panic but `reason == 2`.  Panics when the matrix is not square or a length differs.
    /// `m.set_option("trsv_sweeps", s)` with s >= 0 makes the call apply `m` by s Jacobi sweeps per triangle instead of
    /// the two exact solves (`self` as `m` with s = 0: Jacobi).
    pub fn solve(&self, method: c_int, m: Option<&DeviceCsc<T>>, b: &[T], x: &mut [T], tol: f64, maxit: u64) -> ffi::spal_krylov_info
    where T: HipKrylov {
        let mut info = ffi::spal_krylov_info::default();
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csc_krylov(self.h, method, mh, b, x, tol, maxit, &mut info)); }
        info
    }

    /// X with A X = B for a row-major block of `k` right-hand sides (`b` and `x` hold nrows * k elements, element (i, j)
    /// at i * k + j; `x` holds X0 on entry): k independent CG / BiCGStab iterations in lockstep on shared launches
    /// (spal_csc_krylov_block_*).  Column j and record j are bit for bit `solve`'s loop on column j, whatever k and the
    /// other columns are; a column that has stopped is frozen while the others run on.  Panics as `solve` does, and when
    /// k == 0 or a block is not nrows x k.
    pub fn solve_block(&self, method: c_int, m: Option<&DeviceCsc<T>>, k: usize, b: &[T], x: &mut [T], tol: f64, maxit: u64)
        -> Vec<ffi::spal_krylov_info>
    where T: HipKrylov {
        assert!(k > 0 && b.len() % k == 0 && x.len() == b.len());
        let mut info = vec![ffi::spal_krylov_info::default(); k];
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csc_krylov_block(self.h, method, mh, k as u64, b, x, tol, maxit, info.as_mut_ptr())); }
        info
    }

    /// x with A x = b by restarted GMRES(`restart`, 1 ..= 256), right-preconditioned by `m` as `solve` is; for matrices
    /// that are not symmetric.  Bit for bit the text of include/spal.h; reasons 0 and 1 are decided on the true residual.
    pub fn gmres(&self, m: Option<&DeviceCsc<T>>, b: &[T], x: &mut [T], restart: u64, tol: f64, maxit: u64) -> ffi::spal_krylov_info
    where T: HipKrylov {
        let mut info = ffi::spal_krylov_info::default();
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csc_gmres(self.h, mh, b, x, restart, tol, maxit, &mut info)); }
        info
    }

    /// X with A X = B for a row-major block of `k` right-hand sides by restarted GMRES(`restart`): k independent
    /// iterations in lockstep on shared launches, with cycles common to the block (spal_csc_gmres_block_*).  `b` and `x`
    /// hold nrows * k elements, element (i, j) at i * k + j; `x` holds X0 on entry.  Column j and record j are bit for
    /// bit `gmres`'s text on column j, whatever k and the other columns are.  Panics as `gmres` does, and when k == 0 or a
    /// block is not nrows x k.
    pub fn gmres_block(&self, m: Option<&DeviceCsc<T>>, k: usize, b: &[T], x: &mut [T], restart: u64, tol: f64, maxit: u64)
        -> Vec<ffi::spal_krylov_info>
    where T: HipKrylov {
        assert!(k > 0 && b.len() % k == 0 && x.len() == b.len());
        let mut info = vec![ffi::spal_krylov_info::default(); k];
        let mh = m.map_or(std::ptr::null_mut(), |f| f.h);
        unsafe { ffi::check(T::csc_gmres_block(self.h, mh, k as u64, b, x, restart, tol, maxit, info.as_mut_ptr())); }
        info
    }

    /// `solve_triangular` on device pointers (`x_dev == b_dev` solves in place), enqueued on `stream` and not
    /// synchronised once the triangle has its plan (`trsv_analyse`, or the first solve, builds it).
    ///
    /// # Safety
    /// `b_dev` and `x_dev` must hold `nrows` elements each.
    pub unsafe fn solve_triangular_dev(&self, lower: bool, unit_diagonal: bool, b_dev: *const T, x_dev: *mut T, stream: *mut c_void)
    where T: HipTrsv {
        ffi::check(T::csc_trsv_dev(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, b_dev, x_dev, stream));
    }

    /// `sweeps` Jacobi passes `x <- D^-1 (b - N x)` on the chosen triangle instead of the substitution: an approximate
    /// solve whose every pass is one launch of independent rows.  Bit for bit the sequential text of include/spal.h;
    /// from `sweeps = levels - 1` on it is `solve_triangular`'s result.  No host analysis.  Panics as `solve_triangular`.
    pub fn solve_triangular_sweeps(&self, b: &[T], lower: bool, unit_diagonal: bool, sweeps: u64) -> Vec<T> where T: HipTrsv {
        let (nrows, _, _) = self.shape();
        assert_eq!(nrows, b.len());
        let mut x = vec![T::zero(); nrows];
        unsafe { ffi::check(T::csc_trsv_sweep(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, sweeps, b, &mut x)); }
        x
    }

    /// `solve_triangular_sweeps` on device pointers (`x_dev == b_dev` is allowed), enqueued on `stream` and not
    /// synchronised once the handle is prepared (the first sweep call prepares it); scratch comes and goes in stream order.
    ///
    /// # Safety
    /// `b_dev` and `x_dev` must hold `nrows` elements each.
    pub unsafe fn solve_triangular_sweeps_dev(&self, lower: bool, unit_diagonal: bool, sweeps: u64, b_dev: *const T, x_dev: *mut T,
                                              stream: *mut c_void)
    where T: HipTrsv {
        ffi::check(T::csc_trsv_sweep_dev(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, sweeps, b_dev, x_dev, stream));
    }

    /// Builds the solve plan of one triangle now (host level analysis; synchronises `stream`).
    pub fn trsv_analyse(&self, lower: bool, unit_diagonal: bool, stream: *mut c_void) {
        unsafe { ffi::check(ffi::spal_csc_trsv_analyse(self.h, if lower { 0 } else { 1 }, unit_diagonal as c_int, stream)); }
    }

    /// "kernel" = 1: atomic scatter, 2 (default): converted to CSR on the device once, deterministic.
    pub fn set_option(&self, key: &str, value: i64) {
        let k = std::ffi::CString::new(key).expect("option key");
        unsafe { ffi::check(ffi::spal_csc_set_option(self.h, k.as_ptr(), value)); }
    }

    pub fn download(&self) -> CscMatrix<T> {
        let (nr, nc, nz) = self.shape();
        let (mut colptr, mut rowind, mut values) = (vec![0usize; nc + 1], vec![0usize; nz], vec![T::zero(); nz]);
        unsafe { ffi::check(T::csc_download(self.h, &mut colptr, &mut rowind, &mut values)); }
        CscMatrix::new(nr, nc, colptr, rowind, values)
    }

    /// Device twin of `impl From<&CscMatrix<T>> for CsrMatrix<T>` (src/csr/conv/csc.rs:4-52).
    pub fn to_csr(&self) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_to_csr(self.h, &mut out)); }
        DeviceCsr::from_raw(out)
    }

    /// Device twin of `impl Mul for &CscMatrix<T>` (src/csc/ops/mul.rs:5-60), bit-identical.
    pub fn mul_mat(&self, rhs: &DeviceCsc<T>, stream: *mut c_void) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_mul(self.h, rhs.h, stream, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }

    /// Device twins of `impl Add / Sub / Neg for &CscMatrix<T>` (src/csc/ops/{add,sub,neg}.rs), bit-identical.
    pub fn add_mat(&self, rhs: &DeviceCsc<T>, stream: *mut c_void) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_add(self.h, rhs.h, stream, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }
    pub fn sub_mat(&self, rhs: &DeviceCsc<T>, stream: *mut c_void) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_sub(self.h, rhs.h, stream, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }
    pub fn neg_mat(&self, stream: *mut c_void) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_neg(self.h, stream, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }

    /// The ILU(0) factor (spal_csc_ilu0): as `DeviceCsr::ilu0`, factorised on the CSR twin and returned by columns.
    pub fn ilu0(&self, stream: *mut c_void) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_ilu0(self.h, stream, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }

    /// The greedy colouring of the graph of A + A^T by hashed priority (include/spal.h): exactly the
    /// sequential text, by Jones-Plassmann rounds on the device.  Returns `(colours, ncolours, rounds)`.
    pub fn colour(&self, seed: u64, stream: *mut c_void) -> (Vec<usize>, usize, usize) {
        let (nrows, _, _) = self.shape();
        let mut colours = vec![0u64; nrows];
        let (mut nc, mut rounds) = (0u64, 0u64);
        unsafe { ffi::check(ffi::spal_csc_colour(self.h, seed, stream, colours.as_mut_ptr(), &mut nc, &mut rounds)); }
        (colours.into_iter().map(|c| c as usize).collect(), nc as usize, rounds as usize)
    }

    /// `B = P A P^T`, `B[i'][j'] = A[perm[i']][perm[j']]`, for any permutation `perm` (new -> old); values are moved.
    /// The result keeps `perm` (`ordering`, `permute_vec_dev`).  Panics when `perm` is no permutation of `0..nrows`.
    pub fn permute(&self, perm: &[usize], stream: *mut c_void) -> DeviceCsc<T> {
        let p: Vec<u64> = perm.iter().map(|&i| i as u64).collect();
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_csc_permute(self.h, p.as_ptr(), p.len() as u64, stream, &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }

    /// colour -> order by (colour, row) -> permute on the device: both triangles of the result, and of its `ilu0`,
    /// have at most `ordering().1` levels.
    pub fn multicolour(&self, seed: u64, stream: *mut c_void) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        let mut nc = 0u64;
        unsafe { ffi::check(ffi::spal_csc_multicolour(self.h, seed, stream, &mut out, &mut nc)); }
        DeviceCsc { h: out, _t: PhantomData }
    }

    /// `(perm, ncolours)` of a handle made by `permute` (`ncolours == 0`) or `multicolour`; panics on any other handle.
    pub fn ordering(&self) -> (Vec<usize>, usize) {
        let (nrows, _, _) = self.shape();
        let mut perm = vec![0u64; nrows];
        let mut nc = 0u64;
        unsafe { ffi::check(ffi::spal_csc_ordering(self.h, perm.as_mut_ptr(), &mut nc)); }
        (perm.into_iter().map(|i| i as usize).collect(), nc as usize)
    }

    /// `y[i'] = x[perm[i']]` (into this handle's order), or with `back` `y[perm[i']] = x[i']`; enqueued on `stream`.
    ///
    /// # Safety
    /// `x_dev` and `y_dev` must hold `nrows` elements each and must not be the same vector.
    pub unsafe fn permute_vec_dev(&self, x_dev: *const T, y_dev: *mut T, back: bool, stream: *mut c_void) {
        if std::mem::size_of::<T>() == 8 {
            ffi::check(ffi::spal_csc_permute_vec_dev_f64(self.h, x_dev as *const f64, y_dev as *mut f64, back as c_int, stream));
        } else {
            ffi::check(ffi::spal_csc_permute_vec_dev_f32(self.h, x_dev as *const f32, y_dev as *mut f32, back as c_int, stream));
        }
    }
}

impl<T: HipScalar> DeviceCoo<T> {
    /// Uploads the triplets in insertion order.  `Vec<(usize, usize, T)>` has no guaranteed layout, so `iter()`
    /// (src/coo.rs:491) is unzipped into three arrays; bounds are re-checked (src/coo.rs:432-433).
    pub fn new(coo: &CooMatrix<T>, device: i32) -> Self {
        let (mut r, mut c, mut v) = (Vec::new(), Vec::new(), Vec::new());
        for (row, col, val) in coo.iter() {
            r.push(row);
            c.push(col);
            v.push(*val);
        }
        let mut h = std::ptr::null_mut();
        unsafe { ffi::check(T::coo_upload(device as c_int, coo.nrows() as u64, coo.ncols() as u64, &r, &c, &v, &mut h)); }
        DeviceCoo { h, _t: PhantomData }
    }

    /// Device twin of `impl From<&CooMatrix<T>> for CsrMatrix<T>` (src/csr/conv/coo.rs:4-115): stable order by
    /// (row, col), duplicates summed left to right in insertion order, results equal to zero dropped --
    /// rowptr, colind and values bit-identical to the reference's.
    pub fn assemble_csr(&self) -> DeviceCsr<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_coo_assemble_csr(self.h, std::ptr::null_mut(), &mut out)); }
        DeviceCsr::from_raw(out)
    }

    /// ... and of `impl From<&CooMatrix<T>> for CscMatrix<T>` (src/csc/conv/coo.rs:4-115).
    pub fn assemble_csc(&self) -> DeviceCsc<T> {
        let mut out = std::ptr::null_mut();
        unsafe { ffi::check(ffi::spal_coo_assemble_csc(self.h, std::ptr::null_mut(), &mut out)); }
        DeviceCsc { h: out, _t: PhantomData }
    }
}

//! Per-`Scalar` dispatch to the two instantiations of the C ABI (`Scalar` is implemented for f32 and f64
//! only, src/scalar.rs:56-57).  The crate has no dependencies (Cargo.toml:13), so the entry points are passed
//! to the macro by name instead of being pasted together.
use std::os::raw::{c_int, c_void};

use super::ffi;
use crate::scalar::Scalar;

#[allow(clippy::too_many_arguments)]
pub trait HipScalar: Scalar {
    unsafe fn csr_create(d: c_int, nr: u64, nc: u64, rp: &[usize], ci: &[usize], v: &[Self], out: *mut *mut ffi::spal_csr) -> c_int;
    unsafe fn csr_spmv(a: *mut ffi::spal_csr, x: &[Self], y: &mut [Self]) -> c_int;
    unsafe fn csr_spmv_dev(a: *mut ffi::spal_csr, x: *const Self, y: *mut Self, stream: *mut c_void) -> c_int;
    unsafe fn csr_autotune(a: *mut ffi::spal_csr, x: *const Self, y: *mut Self, stream: *mut c_void, iters: c_int) -> c_int;
    unsafe fn csr_download(a: *mut ffi::spal_csr, rp: &mut [usize], ci: &mut [usize], v: &mut [Self]) -> c_int;
    unsafe fn csc_create(d: c_int, nr: u64, nc: u64, cp: &[usize], ri: &[usize], v: &[Self], out: *mut *mut ffi::spal_csc) -> c_int;
    unsafe fn csc_spmv(a: *mut ffi::spal_csc, x: &[Self], y: &mut [Self]) -> c_int;
    unsafe fn csc_spmv_dev(a: *mut ffi::spal_csc, x: *const Self, y: *mut Self, stream: *mut c_void) -> c_int;
    unsafe fn csc_download(a: *mut ffi::spal_csc, cp: &mut [usize], ri: &mut [usize], v: &mut [Self]) -> c_int;
    unsafe fn coo_upload(d: c_int, nr: u64, nc: u64, r: &[usize], c: &[usize], v: &[Self], out: *mut *mut ffi::spal_coo) -> c_int;
    unsafe fn mg_csr_create(ctx: *mut ffi::spal_mg, nr: u64, nc: u64, rp: &[usize], ci: &[usize], v: &[Self], out: *mut *mut ffi::spal_mg_csr) -> c_int;
    unsafe fn mg_csr_spmv(a: *mut ffi::spal_mg_csr, x: &[Self], y: &mut [Self]) -> c_int;
}

macro_rules! impl_hip_scalar {
    ($t:ty, $csr_create:ident, $csr_spmv:ident, $csr_spmv_dev:ident, $csr_autotune:ident, $csr_download:ident,
     $csc_create:ident, $csc_spmv:ident, $csc_spmv_dev:ident, $csc_download:ident, $coo_upload:ident,
     $mg_csr_create:ident, $mg_csr_spmv:ident) => {
        impl HipScalar for $t {
            unsafe fn csr_create(d: c_int, nr: u64, nc: u64, rp: &[usize], ci: &[usize], v: &[Self], out: *mut *mut ffi::spal_csr) -> c_int {
                ffi::$csr_create(d, nr, nc, rp.as_ptr() as *const u64, rp.len() as u64, ci.as_ptr() as *const u64,
                                 ci.len() as u64, v.as_ptr(), v.len() as u64, out)
            }
            unsafe fn csr_spmv(a: *mut ffi::spal_csr, x: &[Self], y: &mut [Self]) -> c_int {
                ffi::$csr_spmv(a, x.as_ptr(), x.len() as u64, y.as_mut_ptr(), y.len() as u64)
            }
            unsafe fn csr_spmv_dev(a: *mut ffi::spal_csr, x: *const Self, y: *mut Self, stream: *mut c_void) -> c_int {
                ffi::$csr_spmv_dev(a, x, y, stream)
            }
            unsafe fn csr_autotune(a: *mut ffi::spal_csr, x: *const Self, y: *mut Self, stream: *mut c_void, iters: c_int) -> c_int {
                ffi::$csr_autotune(a, x, y, stream, iters)
            }
            unsafe fn csr_download(a: *mut ffi::spal_csr, rp: &mut [usize], ci: &mut [usize], v: &mut [Self]) -> c_int {
                ffi::$csr_download(a, rp.as_mut_ptr() as *mut u64, ci.as_mut_ptr() as *mut u64, v.as_mut_ptr())
            }
            unsafe fn csc_create(d: c_int, nr: u64, nc: u64, cp: &[usize], ri: &[usize], v: &[Self], out: *mut *mut ffi::spal_csc) -> c_int {
                ffi::$csc_create(d, nr, nc, cp.as_ptr() as *const u64, cp.len() as u64, ri.as_ptr() as *const u64,
                                 ri.len() as u64, v.as_ptr(), v.len() as u64, out)
            }
            unsafe fn csc_spmv(a: *mut ffi::spal_csc, x: &[Self], y: &mut [Self]) -> c_int {
                ffi::$csc_spmv(a, x.as_ptr(), x.len() as u64, y.as_mut_ptr(), y.len() as u64)
            }
            unsafe fn csc_spmv_dev(a: *mut ffi::spal_csc, x: *const Self, y: *mut Self, stream: *mut c_void) -> c_int {
                ffi::$csc_spmv_dev(a, x, y, stream)
            }
            unsafe fn csc_download(a: *mut ffi::spal_csc, cp: &mut [usize], ri: &mut [usize], v: &mut [Self]) -> c_int {
                ffi::$csc_download(a, cp.as_mut_ptr() as *mut u64, ri.as_mut_ptr() as *mut u64, v.as_mut_ptr())
            }
            unsafe fn coo_upload(d: c_int, nr: u64, nc: u64, r: &[usize], c: &[usize], v: &[Self], out: *mut *mut ffi::spal_coo) -> c_int {
                ffi::$coo_upload(d, nr, nc, v.len() as u64, r.as_ptr() as *const u64, c.as_ptr() as *const u64, v.as_ptr(), out)
            }
            unsafe fn mg_csr_create(ctx: *mut ffi::spal_mg, nr: u64, nc: u64, rp: &[usize], ci: &[usize], v: &[Self], out: *mut *mut ffi::spal_mg_csr) -> c_int {
                ffi::$mg_csr_create(ctx, nr, nc, rp.as_ptr() as *const u64, rp.len() as u64, ci.as_ptr() as *const u64,
                                    ci.len() as u64, v.as_ptr(), v.len() as u64, out)
            }
            unsafe fn mg_csr_spmv(a: *mut ffi::spal_mg_csr, x: &[Self], y: &mut [Self]) -> c_int {
                ffi::$mg_csr_spmv(a, x.as_ptr(), x.len() as u64, y.as_mut_ptr(), y.len() as u64)
            }
        }
    };
}
impl_hip_scalar!(f64, spal_csr_create_f64, spal_csr_spmv_f64, spal_csr_spmv_dev_f64, spal_csr_autotune_f64,
                 spal_csr_download_f64, spal_csc_create_f64, spal_csc_spmv_f64, spal_csc_spmv_dev_f64,
                 spal_csc_download_f64, spal_coo_upload_f64, spal_mg_csr_create_f64, spal_mg_csr_spmv_f64);
impl_hip_scalar!(f32, spal_csr_create_f32, spal_csr_spmv_f32, spal_csr_spmv_dev_f32, spal_csr_autotune_f32,
                 spal_csr_download_f32, spal_csc_create_f32, spal_csc_spmv_f32, spal_csc_spmv_dev_f32,
                 spal_csc_download_f32, spal_coo_upload_f32, spal_mg_csr_create_f32, spal_mg_csr_spmv_f32);

/// Y = A * X for a dense row-major block (the spal_*_spmm_* entry points): `x` is ncols x k with leading dimension
/// `ldx`, `y` nrows x k with `ldy`.
#[allow(clippy::too_many_arguments)]
pub trait HipSpmm: HipScalar {
    unsafe fn csr_spmm(a: *mut ffi::spal_csr, k: u64, x: &[Self], ldx: u64, x_rows: u64, y: &mut [Self], ldy: u64, y_rows: u64) -> c_int;
    unsafe fn csr_spmm_dev(a: *mut ffi::spal_csr, k: u64, x: *const Self, ldx: u64, y: *mut Self, ldy: u64, stream: *mut c_void) -> c_int;
    unsafe fn csc_spmm(a: *mut ffi::spal_csc, k: u64, x: &[Self], ldx: u64, x_rows: u64, y: &mut [Self], ldy: u64, y_rows: u64) -> c_int;
    unsafe fn csc_spmm_dev(a: *mut ffi::spal_csc, k: u64, x: *const Self, ldx: u64, y: *mut Self, ldy: u64, stream: *mut c_void) -> c_int;
}

macro_rules! impl_hip_spmm {
    ($t:ty, $csr_spmm:ident, $csr_spmm_dev:ident, $csc_spmm:ident, $csc_spmm_dev:ident) => {
        impl HipSpmm for $t {
            unsafe fn csr_spmm(a: *mut ffi::spal_csr, k: u64, x: &[Self], ldx: u64, x_rows: u64, y: &mut [Self], ldy: u64, y_rows: u64) -> c_int {
                ffi::$csr_spmm(a, k, x.as_ptr(), ldx, x_rows, y.as_mut_ptr(), ldy, y_rows)
            }
            unsafe fn csr_spmm_dev(a: *mut ffi::spal_csr, k: u64, x: *const Self, ldx: u64, y: *mut Self, ldy: u64, stream: *mut c_void) -> c_int {
                ffi::$csr_spmm_dev(a, k, x, ldx, y, ldy, stream)
            }
            unsafe fn csc_spmm(a: *mut ffi::spal_csc, k: u64, x: &[Self], ldx: u64, x_rows: u64, y: &mut [Self], ldy: u64, y_rows: u64) -> c_int {
                ffi::$csc_spmm(a, k, x.as_ptr(), ldx, x_rows, y.as_mut_ptr(), ldy, y_rows)
            }
            unsafe fn csc_spmm_dev(a: *mut ffi::spal_csc, k: u64, x: *const Self, ldx: u64, y: *mut Self, ldy: u64, stream: *mut c_void) -> c_int {
                ffi::$csc_spmm_dev(a, k, x, ldx, y, ldy, stream)
            }
        }
    };
}
impl_hip_spmm!(f64, spal_csr_spmm_f64, spal_csr_spmm_dev_f64, spal_csc_spmm_f64, spal_csc_spmm_dev_f64);
impl_hip_spmm!(f32, spal_csr_spmm_f32, spal_csr_spmm_dev_f32, spal_csc_spmm_f32, spal_csc_spmm_dev_f32);

/// L x = b / U x = b (the spal_*_trsv_* entry points): `uplo` 0 lower / 1 upper, `unit_diag` 0 / 1.
pub trait HipTrsv: HipScalar {
    unsafe fn csr_trsv(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, b: &[Self], x: &mut [Self]) -> c_int;
    unsafe fn csr_trsv_dev(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int;
    unsafe fn csc_trsv(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, b: &[Self], x: &mut [Self]) -> c_int;
    unsafe fn csc_trsv_dev(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int;
    // `sweeps` Jacobi passes on the triangle instead of the substitution (the spal_*_trsv_sweep_* entry points)
    unsafe fn csr_trsv_sweep(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b: &[Self], x: &mut [Self]) -> c_int;
    unsafe fn csr_trsv_sweep_dev(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int;
    unsafe fn csc_trsv_sweep(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b: &[Self], x: &mut [Self]) -> c_int;
    unsafe fn csc_trsv_sweep_dev(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int;
}

macro_rules! impl_hip_trsv {
    ($t:ty, $csr_trsv:ident, $csr_trsv_dev:ident, $csc_trsv:ident, $csc_trsv_dev:ident,
     $csr_sweep:ident, $csr_sweep_dev:ident, $csc_sweep:ident, $csc_sweep_dev:ident) => {
        impl HipTrsv for $t {
            unsafe fn csr_trsv(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, b: &[Self], x: &mut [Self]) -> c_int {
                ffi::$csr_trsv(a, uplo, unit_diag, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64)
            }
            unsafe fn csr_trsv_dev(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int {
                ffi::$csr_trsv_dev(a, uplo, unit_diag, b, x, stream)
            }
            unsafe fn csc_trsv(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, b: &[Self], x: &mut [Self]) -> c_int {
                ffi::$csc_trsv(a, uplo, unit_diag, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64)
            }
            unsafe fn csc_trsv_dev(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int {
                ffi::$csc_trsv_dev(a, uplo, unit_diag, b, x, stream)
            }
            unsafe fn csr_trsv_sweep(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b: &[Self], x: &mut [Self]) -> c_int {
                ffi::$csr_sweep(a, uplo, unit_diag, sweeps, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64)
            }
            unsafe fn csr_trsv_sweep_dev(a: *mut ffi::spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int {
                ffi::$csr_sweep_dev(a, uplo, unit_diag, sweeps, b, x, stream)
            }
            unsafe fn csc_trsv_sweep(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b: &[Self], x: &mut [Self]) -> c_int {
                ffi::$csc_sweep(a, uplo, unit_diag, sweeps, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64)
            }
            unsafe fn csc_trsv_sweep_dev(a: *mut ffi::spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const Self, x: *mut Self, stream: *mut c_void) -> c_int {
                ffi::$csc_sweep_dev(a, uplo, unit_diag, sweeps, b, x, stream)
            }
        }
    };
}
impl_hip_trsv!(f64, spal_csr_trsv_f64, spal_csr_trsv_dev_f64, spal_csc_trsv_f64, spal_csc_trsv_dev_f64,
               spal_csr_trsv_sweep_f64, spal_csr_trsv_sweep_dev_f64, spal_csc_trsv_sweep_f64, spal_csc_trsv_sweep_dev_f64);
impl_hip_trsv!(f32, spal_csr_trsv_f32, spal_csr_trsv_dev_f32, spal_csc_trsv_f32, spal_csc_trsv_dev_f32,
               spal_csr_trsv_sweep_f32, spal_csr_trsv_sweep_dev_f32, spal_csc_trsv_sweep_f32, spal_csc_trsv_sweep_dev_f32);

/// CG / BiCGStab and their dot product (the spal_*_krylov_* and spal_dot_* entry points): `method` is
/// `ffi::SPAL_KRYLOV_CG` / `ffi::SPAL_KRYLOV_BICGSTAB`, `m` an ILU(0) factor handle or null.
pub trait HipKrylov: Sized {
    unsafe fn csr_krylov(a: *mut ffi::spal_csr, method: c_int, m: *mut ffi::spal_csr, b: &[Self], x: &mut [Self], tol: f64,
                         maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    unsafe fn csc_krylov(a: *mut ffi::spal_csc, method: c_int, m: *mut ffi::spal_csc, b: &[Self], x: &mut [Self], tol: f64,
                         maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    unsafe fn dot(a: &[Self], b: &[Self], out: *mut Self) -> c_int;
    /// the same two loops on a row-major block of k right-hand sides (the spal_*_krylov_block_* entry points): `b` and
    /// `x` hold nrows * k elements, element (i, j) at i * k + j; `info` points to k records
    unsafe fn csr_krylov_block(a: *mut ffi::spal_csr, method: c_int, m: *mut ffi::spal_csr, k: u64, b: &[Self], x: &mut [Self],
                               tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    unsafe fn csc_krylov_block(a: *mut ffi::spal_csc, method: c_int, m: *mut ffi::spal_csc, k: u64, b: &[Self], x: &mut [Self],
                               tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    /// restarted GMRES (the spal_*_gmres_* entry points): `restart` is 1 ..= 256
    unsafe fn csr_gmres(a: *mut ffi::spal_csr, m: *mut ffi::spal_csr, b: &[Self], x: &mut [Self], restart: u64, tol: f64,
                        maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    unsafe fn csc_gmres(a: *mut ffi::spal_csc, m: *mut ffi::spal_csc, b: &[Self], x: &mut [Self], restart: u64, tol: f64,
                        maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    /// GMRES on a row-major block of k right-hand sides (the spal_*_gmres_block_* entry points): `b` and `x` hold
    /// nrows * k elements, element (i, j) at i * k + j; `info` points to k records
    unsafe fn csr_gmres_block(a: *mut ffi::spal_csr, m: *mut ffi::spal_csr, k: u64, b: &[Self], x: &mut [Self], restart: u64,
                              tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
    unsafe fn csc_gmres_block(a: *mut ffi::spal_csc, m: *mut ffi::spal_csc, k: u64, b: &[Self], x: &mut [Self], restart: u64,
                              tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int;
}

macro_rules! impl_hip_krylov {
    ($t:ty, $csr_krylov:ident, $csc_krylov:ident, $dot:ident, $csr_gmres:ident, $csc_gmres:ident, $csr_block:ident,
     $csc_block:ident, $csr_gmres_block:ident, $csc_gmres_block:ident) => {
        impl HipKrylov for $t {
            unsafe fn csr_gmres_block(a: *mut ffi::spal_csr, m: *mut ffi::spal_csr, k: u64, b: &[Self], x: &mut [Self],
                                      restart: u64, tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                let (br, xr) = (if k > 0 { b.len() as u64 / k } else { 0 }, if k > 0 { x.len() as u64 / k } else { 0 });
                ffi::$csr_gmres_block(a, m, k, b.as_ptr(), k, br, x.as_mut_ptr(), k, xr, restart, tol, maxit, info)
            }
            unsafe fn csc_gmres_block(a: *mut ffi::spal_csc, m: *mut ffi::spal_csc, k: u64, b: &[Self], x: &mut [Self],
                                      restart: u64, tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                let (br, xr) = (if k > 0 { b.len() as u64 / k } else { 0 }, if k > 0 { x.len() as u64 / k } else { 0 });
                ffi::$csc_gmres_block(a, m, k, b.as_ptr(), k, br, x.as_mut_ptr(), k, xr, restart, tol, maxit, info)
            }
            unsafe fn csr_krylov_block(a: *mut ffi::spal_csr, method: c_int, m: *mut ffi::spal_csr, k: u64, b: &[Self],
                                       x: &mut [Self], tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                let (br, xr) = (if k > 0 { b.len() as u64 / k } else { 0 }, if k > 0 { x.len() as u64 / k } else { 0 });
                ffi::$csr_block(a, method, m, k, b.as_ptr(), k, br, x.as_mut_ptr(), k, xr, tol, maxit, info)
            }
            unsafe fn csc_krylov_block(a: *mut ffi::spal_csc, method: c_int, m: *mut ffi::spal_csc, k: u64, b: &[Self],
                                       x: &mut [Self], tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                let (br, xr) = (if k > 0 { b.len() as u64 / k } else { 0 }, if k > 0 { x.len() as u64 / k } else { 0 });
                ffi::$csc_block(a, method, m, k, b.as_ptr(), k, br, x.as_mut_ptr(), k, xr, tol, maxit, info)
            }
            unsafe fn csr_krylov(a: *mut ffi::spal_csr, method: c_int, m: *mut ffi::spal_csr, b: &[Self], x: &mut [Self],
                                 tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                ffi::$csr_krylov(a, method, m, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64, tol, maxit, info)
            }
            unsafe fn csc_krylov(a: *mut ffi::spal_csc, method: c_int, m: *mut ffi::spal_csc, b: &[Self], x: &mut [Self],
                                 tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                ffi::$csc_krylov(a, method, m, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64, tol, maxit, info)
            }
            unsafe fn dot(a: &[Self], b: &[Self], out: *mut Self) -> c_int {
                ffi::$dot(a.as_ptr(), b.as_ptr(), a.len() as u64, out)
            }
            unsafe fn csr_gmres(a: *mut ffi::spal_csr, m: *mut ffi::spal_csr, b: &[Self], x: &mut [Self], restart: u64,
                                tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                ffi::$csr_gmres(a, m, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64, restart, tol, maxit, info)
            }
            unsafe fn csc_gmres(a: *mut ffi::spal_csc, m: *mut ffi::spal_csc, b: &[Self], x: &mut [Self], restart: u64,
                                tol: f64, maxit: u64, info: *mut ffi::spal_krylov_info) -> c_int {
                ffi::$csc_gmres(a, m, b.as_ptr(), b.len() as u64, x.as_mut_ptr(), x.len() as u64, restart, tol, maxit, info)
            }
        }
    };
}
impl_hip_krylov!(f64, spal_csr_krylov_f64, spal_csc_krylov_f64, spal_dot_f64, spal_csr_gmres_f64, spal_csc_gmres_f64,
                 spal_csr_krylov_block_f64, spal_csc_krylov_block_f64, spal_csr_gmres_block_f64,
                 spal_csc_gmres_block_f64);
impl_hip_krylov!(f32, spal_csr_krylov_f32, spal_csc_krylov_f32, spal_dot_f32, spal_csr_gmres_f32, spal_csc_gmres_f32,
                 spal_csr_krylov_block_f32, spal_csc_krylov_block_f32, spal_csr_gmres_block_f32,
                 spal_csc_gmres_block_f32);

/// dot(a, b) by the library's definition (include/spal.h): products rounded, then the fixed tree over tiles of 1024.
pub fn dot<T: HipKrylov + Default>(a: &[T], b: &[T]) -> T {
    assert_eq!(a.len(), b.len());
    let mut out = T::default();
    unsafe { ffi::check(T::dot(a, b, &mut out)); }
    out
}

//! Raw bindings to libspal_hip.so -- GENERATED from include/spal.h by tools/gen_rust_ffi.py; do not edit.
//!
//! NOT COMPILED IN THIS REPOSITORY'S PIPELINE: the build image has no rustc/cargo.  This is
//! the source a spalinalg maintainer adds to the crate as `src/hip/ffi.rs`; see INTEGRATION.md.  Every
//! function of the C ABI is declared (tests/test_host_abi.py keeps this file in step with the header).
#![allow(non_camel_case_types)]
use std::os::raw::{c_char, c_int, c_void};

#[repr(C)] pub struct spal_csr { _private: [u8; 0] }
#[repr(C)] pub struct spal_csc { _private: [u8; 0] }
#[repr(C)] pub struct spal_coo { _private: [u8; 0] }
#[repr(C)] pub struct spal_mg { _private: [u8; 0] }
#[repr(C)] pub struct spal_mg_csr { _private: [u8; 0] }
#[repr(C)] pub struct spal_amg { _private: [u8; 0] }
#[repr(C)] pub struct spal_fsai { _private: [u8; 0] }

pub const SPAL_OK: c_int = 0;
pub const SPAL_ERR_INVALID_ARGUMENT: c_int = 1;
pub const SPAL_ERR_INVARIANT: c_int = 2;
pub const SPAL_ERR_HIP: c_int = 3;
pub const SPAL_ERR_OUT_OF_MEMORY: c_int = 4;
pub const SPAL_ERR_UNSUPPORTED: c_int = 5;
pub const SPAL_ERR_NO_DEVICE: c_int = 6;
pub const SPAL_ERR_INDEX_OUT_OF_BOUNDS: c_int = 7;

pub const SPAL_KRYLOV_CG: c_int = 0;
pub const SPAL_KRYLOV_BICGSTAB: c_int = 1;
/// What spal_*_krylov_* report: reason 0 converged, 1 maxit reached, 2 breakdown / not finite.
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct spal_krylov_info { pub iterations: u64, pub reason: c_int, pub residual_sq: f64, pub rhs_sq: f64, pub solve_ms: f64 }
/// The parameters of spal_*_amg_setup; spal_amg_default_params fills in {0, 16, 64, 2, 16, 1, 2/3, 1}.
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct spal_amg_params { pub seed: u64, pub max_levels: u64, pub coarse_rows: u64, pub nu: u64, pub coarse_sweeps: u64, pub gamma: u64, pub omega: f64, pub alpha: f64 }
pub const SPAL_EIGSH_LA: c_int = 0;
pub const SPAL_EIGSH_SA: c_int = 1;
/// What spal_*_eigsh_* report: reason 0 converged, 1 maxit restarts, 2 not finite, 3 space exhausted below k.
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct spal_eigsh_info { pub restarts: u64, pub products: u64, pub converged: u64, pub reason: c_int, pub solve_ms: f64 }
/// What spal_*_eigsh_filtered_* report: eigsh's fields, the warm-up's counts, the interval, a0, the degree.
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct spal_eigsh_filter_info { pub restarts: u64, pub products: u64, pub converged: u64, pub reason: c_int, pub solve_ms: f64, pub warm_restarts: u64, pub warm_products: u64, pub lo: f64, pub hi: f64, pub a0: f64, pub degree: u64 }
/// What spal_*_eigsh_near_* report: eigsh's fields, the interval, sigma, its place gamma in [-1, 1], the degree.
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct spal_eigsh_near_info { pub restarts: u64, pub products: u64, pub converged: u64, pub reason: c_int, pub solve_ms: f64, pub lo: f64, pub hi: f64, pub sigma: f64, pub gamma: f64, pub degree: u64 }
/// What spal_*_kpm_moments_* report: the products per column, the interval, Gershgorin's bounds, the degree, the probes.
#[repr(C)] #[derive(Clone, Copy, Debug, Default)]
pub struct spal_kpm_info { pub products: u64, pub lo: f64, pub hi: f64, pub glo: f64, pub ghi: f64, pub degree: u64, pub probes: u64, pub solve_ms: f64 }

#[link(name = "spal_hip")]
extern "C" {
    pub fn spal_last_error() -> *const c_char;
    pub fn spal_version() -> *const c_char;
    pub fn spal_device_count(count: *mut c_int) -> c_int;
    pub fn spal_csr_validate(nrows: u64, ncols: u64, rowptr: *const u64, rowptr_len: u64, colind: *const u64, colind_len: u64, values_len: u64, reason: *mut c_int) -> c_int;
    pub fn spal_csc_validate(nrows: u64, ncols: u64, colptr: *const u64, colptr_len: u64, rowind: *const u64, rowind_len: u64, values_len: u64, reason: *mut c_int) -> c_int;
    pub fn spal_partition_rows(rowptr: *const u64, nrows: u64, nparts: u32, bounds: *mut u64) -> c_int;
    pub fn spal_csr_create_f64(device: c_int, nrows: u64, ncols: u64, rowptr: *const u64, rowptr_len: u64, colind: *const u64, colind_len: u64, values: *const f64, values_len: u64, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csr_create_f32(device: c_int, nrows: u64, ncols: u64, rowptr: *const u64, rowptr_len: u64, colind: *const u64, colind_len: u64, values: *const f32, values_len: u64, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csr_destroy(a: *mut spal_csr) -> c_int;
    pub fn spal_csr_shape(a: *mut spal_csr, nrows: *mut u64, ncols: *mut u64, nnz: *mut u64, elem_size: *mut c_int) -> c_int;
    pub fn spal_csr_spmv_f64(a: *mut spal_csr, x: *const f64, x_len: u64, y: *mut f64, y_len: u64) -> c_int;
    pub fn spal_csr_spmv_f32(a: *mut spal_csr, x: *const f32, x_len: u64, y: *mut f32, y_len: u64) -> c_int;
    pub fn spal_csr_spmv_dev_f64(a: *mut spal_csr, x_dev: *const f64, y_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_spmv_dev_f32(a: *mut spal_csr, x_dev: *const f32, y_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csr_download_f64(a: *mut spal_csr, rowptr: *mut u64, colind: *mut u64, values: *mut f64) -> c_int;
    pub fn spal_csr_download_f32(a: *mut spal_csr, rowptr: *mut u64, colind: *mut u64, values: *mut f32) -> c_int;
    pub fn spal_csr_set_option(a: *mut spal_csr, key: *const c_char, value: i64) -> c_int;
    pub fn spal_csr_autotune_f64(a: *mut spal_csr, x_dev: *const f64, y_dev: *mut f64, stream: *mut c_void, iters: c_int) -> c_int;
    pub fn spal_csr_autotune_f32(a: *mut spal_csr, x_dev: *const f32, y_dev: *mut f32, stream: *mut c_void, iters: c_int) -> c_int;
    pub fn spal_csr_alloc_vectors(a: *mut spal_csr, x_dev: *mut *mut c_void, y_dev: *mut *mut c_void, stream: *mut c_void) -> c_int;
    pub fn spal_csr_describe(a: *mut spal_csr, buf: *mut c_char, buf_len: usize) -> c_int;
    pub fn spal_csc_create_f64(device: c_int, nrows: u64, ncols: u64, colptr: *const u64, colptr_len: u64, rowind: *const u64, rowind_len: u64, values: *const f64, values_len: u64, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csc_create_f32(device: c_int, nrows: u64, ncols: u64, colptr: *const u64, colptr_len: u64, rowind: *const u64, rowind_len: u64, values: *const f32, values_len: u64, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csc_destroy(a: *mut spal_csc) -> c_int;
    pub fn spal_csc_shape(a: *mut spal_csc, nrows: *mut u64, ncols: *mut u64, nnz: *mut u64, elem_size: *mut c_int) -> c_int;
    pub fn spal_csc_spmv_f64(a: *mut spal_csc, x: *const f64, x_len: u64, y: *mut f64, y_len: u64) -> c_int;
    pub fn spal_csc_spmv_f32(a: *mut spal_csc, x: *const f32, x_len: u64, y: *mut f32, y_len: u64) -> c_int;
    pub fn spal_csc_spmv_dev_f64(a: *mut spal_csc, x_dev: *const f64, y_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_spmv_dev_f32(a: *mut spal_csc, x_dev: *const f32, y_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csc_download_f64(a: *mut spal_csc, colptr: *mut u64, rowind: *mut u64, values: *mut f64) -> c_int;
    pub fn spal_csc_download_f32(a: *mut spal_csc, colptr: *mut u64, rowind: *mut u64, values: *mut f32) -> c_int;
    pub fn spal_csc_set_option(a: *mut spal_csc, key: *const c_char, value: i64) -> c_int;
    pub fn spal_csc_autotune_f64(a: *mut spal_csc, x_dev: *const f64, y_dev: *mut f64, stream: *mut c_void, iters: c_int) -> c_int;
    pub fn spal_csc_autotune_f32(a: *mut spal_csc, x_dev: *const f32, y_dev: *mut f32, stream: *mut c_void, iters: c_int) -> c_int;
    pub fn spal_csc_describe(a: *mut spal_csc, buf: *mut c_char, buf_len: usize) -> c_int;
    pub fn spal_csc_status(a: *mut spal_csc, invalid_products: *mut c_int) -> c_int;
    pub fn spal_csr_spmm_f64(a: *mut spal_csr, k: u64, x: *const f64, ldx: u64, x_rows: u64, y: *mut f64, ldy: u64, y_rows: u64) -> c_int;
    pub fn spal_csr_spmm_f32(a: *mut spal_csr, k: u64, x: *const f32, ldx: u64, x_rows: u64, y: *mut f32, ldy: u64, y_rows: u64) -> c_int;
    pub fn spal_csr_spmm_dev_f64(a: *mut spal_csr, k: u64, x_dev: *const f64, ldx: u64, y_dev: *mut f64, ldy: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_spmm_dev_f32(a: *mut spal_csr, k: u64, x_dev: *const f32, ldx: u64, y_dev: *mut f32, ldy: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_spmm_f64(a: *mut spal_csc, k: u64, x: *const f64, ldx: u64, x_rows: u64, y: *mut f64, ldy: u64, y_rows: u64) -> c_int;
    pub fn spal_csc_spmm_f32(a: *mut spal_csc, k: u64, x: *const f32, ldx: u64, x_rows: u64, y: *mut f32, ldy: u64, y_rows: u64) -> c_int;
    pub fn spal_csc_spmm_dev_f64(a: *mut spal_csc, k: u64, x_dev: *const f64, ldx: u64, y_dev: *mut f64, ldy: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_spmm_dev_f32(a: *mut spal_csc, k: u64, x_dev: *const f32, ldx: u64, y_dev: *mut f32, ldy: u64, stream: *mut c_void) -> c_int;
    pub fn spal_trsv_levels(n: u64, rowptr: *const u64, colind: *const u64, uplo: c_int, unit_diag: c_int, level_of: *mut u64, nlevels: *mut u64) -> c_int;
    pub fn spal_csr_trsv_analyse(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsv_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, b: *const f64, b_len: u64, x: *mut f64, x_len: u64) -> c_int;
    pub fn spal_csr_trsv_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, b: *const f32, b_len: u64, x: *mut f32, x_len: u64) -> c_int;
    pub fn spal_csr_trsv_dev_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, b_dev: *const f64, x_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsv_dev_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, b_dev: *const f32, x_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsv_analyse(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsv_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, b: *const f64, b_len: u64, x: *mut f64, x_len: u64) -> c_int;
    pub fn spal_csc_trsv_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, b: *const f32, b_len: u64, x: *mut f32, x_len: u64) -> c_int;
    pub fn spal_csc_trsv_dev_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, b_dev: *const f64, x_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsv_dev_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, b_dev: *const f32, x_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsv_sweep_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const f64, b_len: u64, x: *mut f64, x_len: u64) -> c_int;
    pub fn spal_csr_trsv_sweep_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const f32, b_len: u64, x: *mut f32, x_len: u64) -> c_int;
    pub fn spal_csr_trsv_sweep_dev_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b_dev: *const f64, x_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsv_sweep_dev_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, b_dev: *const f32, x_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsv_sweep_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const f64, b_len: u64, x: *mut f64, x_len: u64) -> c_int;
    pub fn spal_csc_trsv_sweep_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b: *const f32, b_len: u64, x: *mut f32, x_len: u64) -> c_int;
    pub fn spal_csc_trsv_sweep_dev_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b_dev: *const f64, x_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsv_sweep_dev_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, b_dev: *const f32, x_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsm_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csr_trsm_dev_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsm_sweep_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csr_trsm_sweep_dev_f64(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsm_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csr_trsm_dev_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_trsm_sweep_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csr_trsm_sweep_dev_f32(a: *mut spal_csr, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsm_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csc_trsm_dev_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsm_sweep_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csc_trsm_sweep_dev_f64(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsm_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csc_trsm_dev_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_trsm_sweep_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64) -> c_int;
    pub fn spal_csc_trsm_sweep_dev_f32(a: *mut spal_csc, uplo: c_int, unit_diag: c_int, sweeps: u64, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_ilu0(a: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csc_ilu0(a: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csr_ilu0_sweep(a: *mut spal_csr, sweeps: u64, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csc_ilu0_sweep(a: *mut spal_csc, sweeps: u64, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_dot_f64(a: *const f64, b: *const f64, n: u64, out: *mut f64) -> c_int;
    pub fn spal_dot_f32(a: *const f32, b: *const f32, n: u64, out: *mut f32) -> c_int;
    pub fn spal_dot_dev_f64(device: c_int, a_dev: *const f64, b_dev: *const f64, n: u64, out_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_dot_dev_f32(device: c_int, a_dev: *const f32, b_dev: *const f32, n: u64, out_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csr_krylov_f64(a: *mut spal_csr, method: c_int, m: *mut spal_csr, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_f32(a: *mut spal_csr, method: c_int, m: *mut spal_csr, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_dev_f64(a: *mut spal_csr, method: c_int, m: *mut spal_csr, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_dev_f32(a: *mut spal_csr, method: c_int, m: *mut spal_csr, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_f64(a: *mut spal_csc, method: c_int, m: *mut spal_csc, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_f32(a: *mut spal_csc, method: c_int, m: *mut spal_csc, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_dev_f64(a: *mut spal_csc, method: c_int, m: *mut spal_csc, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_dev_f32(a: *mut spal_csc, method: c_int, m: *mut spal_csc, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_block_f64(a: *mut spal_csr, method: c_int, m: *mut spal_csr, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_block_f32(a: *mut spal_csr, method: c_int, m: *mut spal_csr, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_block_dev_f64(a: *mut spal_csr, method: c_int, m: *mut spal_csr, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_block_dev_f32(a: *mut spal_csr, method: c_int, m: *mut spal_csr, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_block_f64(a: *mut spal_csc, method: c_int, m: *mut spal_csc, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_block_f32(a: *mut spal_csc, method: c_int, m: *mut spal_csc, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_block_dev_f64(a: *mut spal_csc, method: c_int, m: *mut spal_csc, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_block_dev_f32(a: *mut spal_csc, method: c_int, m: *mut spal_csc, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_f64(a: *mut spal_csr, m: *mut spal_csr, shift: f64, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_f32(a: *mut spal_csr, m: *mut spal_csr, shift: f64, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_dev_f64(a: *mut spal_csr, m: *mut spal_csr, shift: f64, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_dev_f32(a: *mut spal_csr, m: *mut spal_csr, shift: f64, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_f64(a: *mut spal_csc, m: *mut spal_csc, shift: f64, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_f32(a: *mut spal_csc, m: *mut spal_csc, shift: f64, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_dev_f64(a: *mut spal_csc, m: *mut spal_csc, shift: f64, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_dev_f32(a: *mut spal_csc, m: *mut spal_csc, shift: f64, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_block_f64(a: *mut spal_csr, m: *mut spal_csr, shift: f64, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_block_f32(a: *mut spal_csr, m: *mut spal_csr, shift: f64, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_block_dev_f64(a: *mut spal_csr, m: *mut spal_csr, shift: f64, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_block_dev_f32(a: *mut spal_csr, m: *mut spal_csr, shift: f64, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_block_f64(a: *mut spal_csc, m: *mut spal_csc, shift: f64, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_block_f32(a: *mut spal_csc, m: *mut spal_csc, shift: f64, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_block_dev_f64(a: *mut spal_csc, m: *mut spal_csc, shift: f64, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_block_dev_f32(a: *mut spal_csc, m: *mut spal_csc, shift: f64, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_f64(a: *mut spal_csr, m: *mut spal_csr, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_f32(a: *mut spal_csr, m: *mut spal_csr, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_dev_f64(a: *mut spal_csr, m: *mut spal_csr, b_dev: *const f64, x_dev: *mut f64, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_dev_f32(a: *mut spal_csr, m: *mut spal_csr, b_dev: *const f32, x_dev: *mut f32, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_f64(a: *mut spal_csc, m: *mut spal_csc, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_f32(a: *mut spal_csc, m: *mut spal_csc, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_dev_f64(a: *mut spal_csc, m: *mut spal_csc, b_dev: *const f64, x_dev: *mut f64, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_dev_f32(a: *mut spal_csc, m: *mut spal_csc, b_dev: *const f32, x_dev: *mut f32, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_block_f64(a: *mut spal_csr, m: *mut spal_csr, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_block_f32(a: *mut spal_csr, m: *mut spal_csr, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_block_dev_f64(a: *mut spal_csr, m: *mut spal_csr, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_gmres_block_dev_f32(a: *mut spal_csr, m: *mut spal_csr, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_block_f64(a: *mut spal_csc, m: *mut spal_csc, k: u64, b: *const f64, ldb: u64, b_rows: u64, x: *mut f64, ldx: u64, x_rows: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_block_f32(a: *mut spal_csc, m: *mut spal_csc, k: u64, b: *const f32, ldb: u64, b_rows: u64, x: *mut f32, ldx: u64, x_rows: u64, restart: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_block_dev_f64(a: *mut spal_csc, m: *mut spal_csc, k: u64, b_dev: *const f64, ldb: u64, x_dev: *mut f64, ldx: u64, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_gmres_block_dev_f32(a: *mut spal_csc, m: *mut spal_csc, k: u64, b_dev: *const f32, ldb: u64, x_dev: *mut f32, ldx: u64, restart: u64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_eigsh_jacobi(m: u64, s: *const f64, theta: *mut f64, y: *mut f64, sweeps: *mut u64) -> c_int;
    pub fn spal_csr_eigsh_f64(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0: *const f64, v0_len: u64, seed: u64, tol: f64, maxit: u64, theta: *mut f64, theta_len: u64, resid: *mut f64, resid_len: u64, x: *mut f64, ldx: u64, x_rows: u64, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csr_eigsh_f32(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0: *const f32, v0_len: u64, seed: u64, tol: f64, maxit: u64, theta: *mut f32, theta_len: u64, resid: *mut f32, resid_len: u64, x: *mut f32, ldx: u64, x_rows: u64, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csr_eigsh_dev_f64(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0_dev: *const f64, seed: u64, tol: f64, maxit: u64, theta: *mut f64, resid: *mut f64, x_dev: *mut f64, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csr_eigsh_dev_f32(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0_dev: *const f32, seed: u64, tol: f64, maxit: u64, theta: *mut f32, resid: *mut f32, x_dev: *mut f32, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csc_eigsh_f64(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0: *const f64, v0_len: u64, seed: u64, tol: f64, maxit: u64, theta: *mut f64, theta_len: u64, resid: *mut f64, resid_len: u64, x: *mut f64, ldx: u64, x_rows: u64, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csc_eigsh_f32(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0: *const f32, v0_len: u64, seed: u64, tol: f64, maxit: u64, theta: *mut f32, theta_len: u64, resid: *mut f32, resid_len: u64, x: *mut f32, ldx: u64, x_rows: u64, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csc_eigsh_dev_f64(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0_dev: *const f64, seed: u64, tol: f64, maxit: u64, theta: *mut f64, resid: *mut f64, x_dev: *mut f64, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csc_eigsh_dev_f32(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0_dev: *const f32, seed: u64, tol: f64, maxit: u64, theta: *mut f32, resid: *mut f32, x_dev: *mut f32, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_info) -> c_int;
    pub fn spal_csr_cheb_apply_f64(a: *mut spal_csr, x: *const f64, x_len: u64, out: *mut f64, out_len: u64, degree: u64, lo: f64, hi: f64, a0: f64) -> c_int;
    pub fn spal_csr_cheb_apply_f32(a: *mut spal_csr, x: *const f32, x_len: u64, out: *mut f32, out_len: u64, degree: u64, lo: f64, hi: f64, a0: f64) -> c_int;
    pub fn spal_csr_cheb_apply_dev_f64(a: *mut spal_csr, x_dev: *const f64, out_dev: *mut f64, degree: u64, lo: f64, hi: f64, a0: f64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_cheb_apply_dev_f32(a: *mut spal_csr, x_dev: *const f32, out_dev: *mut f32, degree: u64, lo: f64, hi: f64, a0: f64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_cheb_apply_f64(a: *mut spal_csc, x: *const f64, x_len: u64, out: *mut f64, out_len: u64, degree: u64, lo: f64, hi: f64, a0: f64) -> c_int;
    pub fn spal_csc_cheb_apply_f32(a: *mut spal_csc, x: *const f32, x_len: u64, out: *mut f32, out_len: u64, degree: u64, lo: f64, hi: f64, a0: f64) -> c_int;
    pub fn spal_csc_cheb_apply_dev_f64(a: *mut spal_csc, x_dev: *const f64, out_dev: *mut f64, degree: u64, lo: f64, hi: f64, a0: f64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_cheb_apply_dev_f32(a: *mut spal_csc, x_dev: *const f32, out_dev: *mut f32, degree: u64, lo: f64, hi: f64, a0: f64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_gershgorin(a: *mut spal_csr, glo: *mut f64, ghi: *mut f64) -> c_int;
    pub fn spal_csc_gershgorin(a: *mut spal_csc, glo: *mut f64, ghi: *mut f64) -> c_int;
    pub fn spal_csr_eigsh_filtered_f64(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0: *const f64, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f64, theta_len: u64, resid: *mut f64, resid_len: u64, x: *mut f64, ldx: u64, x_rows: u64, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csr_eigsh_filtered_f32(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0: *const f32, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f32, theta_len: u64, resid: *mut f32, resid_len: u64, x: *mut f32, ldx: u64, x_rows: u64, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csr_eigsh_filtered_dev_f64(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0_dev: *const f64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f64, resid: *mut f64, x_dev: *mut f64, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csr_eigsh_filtered_dev_f32(a: *mut spal_csr, k: u64, which: c_int, ncv: u64, v0_dev: *const f32, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f32, resid: *mut f32, x_dev: *mut f32, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csc_eigsh_filtered_f64(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0: *const f64, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f64, theta_len: u64, resid: *mut f64, resid_len: u64, x: *mut f64, ldx: u64, x_rows: u64, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csc_eigsh_filtered_f32(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0: *const f32, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f32, theta_len: u64, resid: *mut f32, resid_len: u64, x: *mut f32, ldx: u64, x_rows: u64, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csc_eigsh_filtered_dev_f64(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0_dev: *const f64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f64, resid: *mut f64, x_dev: *mut f64, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_csc_eigsh_filtered_dev_f32(a: *mut spal_csc, k: u64, which: c_int, ncv: u64, v0_dev: *const f32, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, warmup: u64, theta: *mut f32, resid: *mut f32, x_dev: *mut f32, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_filter_info) -> c_int;
    pub fn spal_cheb_delta_coefficients(degree: u64, gamma: f64, coef: *mut f64, coef_len: u64) -> c_int;
    pub fn spal_csr_cheb_series_f64(a: *mut spal_csr, x: *const f64, x_len: u64, out: *mut f64, out_len: u64, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64) -> c_int;
    pub fn spal_csr_cheb_series_dev_f64(a: *mut spal_csr, x_dev: *const f64, out_dev: *mut f64, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_cheb_series_f32(a: *mut spal_csr, x: *const f32, x_len: u64, out: *mut f32, out_len: u64, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64) -> c_int;
    pub fn spal_csr_cheb_series_dev_f32(a: *mut spal_csr, x_dev: *const f32, out_dev: *mut f32, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_cheb_series_f64(a: *mut spal_csc, x: *const f64, x_len: u64, out: *mut f64, out_len: u64, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64) -> c_int;
    pub fn spal_csc_cheb_series_dev_f64(a: *mut spal_csc, x_dev: *const f64, out_dev: *mut f64, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csc_cheb_series_f32(a: *mut spal_csc, x: *const f32, x_len: u64, out: *mut f32, out_len: u64, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64) -> c_int;
    pub fn spal_csc_cheb_series_dev_f32(a: *mut spal_csc, x_dev: *const f32, out_dev: *mut f32, degree: u64, lo: f64, hi: f64, coef: *const f64, coef_len: u64, stream: *mut c_void) -> c_int;
    pub fn spal_csr_eigsh_near_f64(a: *mut spal_csr, k: u64, sigma: f64, ncv: u64, v0: *const f64, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f64, theta_len: u64, resid: *mut f64, resid_len: u64, x: *mut f64, ldx: u64, x_rows: u64, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csr_eigsh_near_dev_f64(a: *mut spal_csr, k: u64, sigma: f64, ncv: u64, v0_dev: *const f64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f64, resid: *mut f64, x_dev: *mut f64, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csr_eigsh_near_f32(a: *mut spal_csr, k: u64, sigma: f64, ncv: u64, v0: *const f32, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f32, theta_len: u64, resid: *mut f32, resid_len: u64, x: *mut f32, ldx: u64, x_rows: u64, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csr_eigsh_near_dev_f32(a: *mut spal_csr, k: u64, sigma: f64, ncv: u64, v0_dev: *const f32, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f32, resid: *mut f32, x_dev: *mut f32, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csc_eigsh_near_f64(a: *mut spal_csc, k: u64, sigma: f64, ncv: u64, v0: *const f64, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f64, theta_len: u64, resid: *mut f64, resid_len: u64, x: *mut f64, ldx: u64, x_rows: u64, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csc_eigsh_near_dev_f64(a: *mut spal_csc, k: u64, sigma: f64, ncv: u64, v0_dev: *const f64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f64, resid: *mut f64, x_dev: *mut f64, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csc_eigsh_near_f32(a: *mut spal_csc, k: u64, sigma: f64, ncv: u64, v0: *const f32, v0_len: u64, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f32, theta_len: u64, resid: *mut f32, resid_len: u64, x: *mut f32, ldx: u64, x_rows: u64, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csc_eigsh_near_dev_f32(a: *mut spal_csc, k: u64, sigma: f64, ncv: u64, v0_dev: *const f32, seed: u64, tol: f64, maxit: u64, degree: u64, automatic: c_int, lo: f64, hi: f64, theta: *mut f32, resid: *mut f32, x_dev: *mut f32, ldx: u64, stream: *mut c_void, info: *mut spal_eigsh_near_info) -> c_int;
    pub fn spal_csr_kpm_moments_f64(a: *mut spal_csr, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z: *const f64, z_rows: u64, ldz: u64, mu: *mut f64, mu_len: u64, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csr_kpm_moments_dev_f64(a: *mut spal_csr, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z_dev: *const f64, ldz: u64, mu: *mut f64, mu_len: u64, stream: *mut c_void, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csr_kpm_moments_f32(a: *mut spal_csr, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z: *const f32, z_rows: u64, ldz: u64, mu: *mut f64, mu_len: u64, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csr_kpm_moments_dev_f32(a: *mut spal_csr, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z_dev: *const f32, ldz: u64, mu: *mut f64, mu_len: u64, stream: *mut c_void, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csc_kpm_moments_f64(a: *mut spal_csc, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z: *const f64, z_rows: u64, ldz: u64, mu: *mut f64, mu_len: u64, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csc_kpm_moments_dev_f64(a: *mut spal_csc, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z_dev: *const f64, ldz: u64, mu: *mut f64, mu_len: u64, stream: *mut c_void, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csc_kpm_moments_f32(a: *mut spal_csc, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z: *const f32, z_rows: u64, ldz: u64, mu: *mut f64, mu_len: u64, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_csc_kpm_moments_dev_f32(a: *mut spal_csc, degree: u64, k: u64, seed: u64, automatic: c_int, lo: f64, hi: f64, z_dev: *const f32, ldz: u64, mu: *mut f64, mu_len: u64, stream: *mut c_void, info: *mut spal_kpm_info) -> c_int;
    pub fn spal_colour_greedy(n: u64, rowptr: *const u64, colind: *const u64, seed: u64, colour: *mut u64, ncolours: *mut u64) -> c_int;
    pub fn spal_perm_from_colours(n: u64, colour: *const u64, perm: *mut u64) -> c_int;
    pub fn spal_csr_colour(a: *mut spal_csr, seed: u64, stream: *mut c_void, colour_host: *mut u64, ncolours: *mut u64, rounds: *mut u64) -> c_int;
    pub fn spal_csc_colour(a: *mut spal_csc, seed: u64, stream: *mut c_void, colour_host: *mut u64, ncolours: *mut u64, rounds: *mut u64) -> c_int;
    pub fn spal_csr_permute(a: *mut spal_csr, perm_host: *const u64, n: u64, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csc_permute(a: *mut spal_csc, perm_host: *const u64, n: u64, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csr_multicolour(a: *mut spal_csr, seed: u64, stream: *mut c_void, out: *mut *mut spal_csr, ncolours: *mut u64) -> c_int;
    pub fn spal_csc_multicolour(a: *mut spal_csc, seed: u64, stream: *mut c_void, out: *mut *mut spal_csc, ncolours: *mut u64) -> c_int;
    pub fn spal_csr_ordering(a: *mut spal_csr, perm_host: *mut u64, ncolours: *mut u64) -> c_int;
    pub fn spal_csc_ordering(a: *mut spal_csc, perm_host: *mut u64, ncolours: *mut u64) -> c_int;
    pub fn spal_csr_permute_vec_f64(a: *mut spal_csr, x: *const f64, x_len: u64, y: *mut f64, y_len: u64, direction: c_int) -> c_int;
    pub fn spal_csr_permute_vec_f32(a: *mut spal_csr, x: *const f32, x_len: u64, y: *mut f32, y_len: u64, direction: c_int) -> c_int;
    pub fn spal_csr_permute_vec_dev_f64(a: *mut spal_csr, x_dev: *const f64, y_dev: *mut f64, direction: c_int, stream: *mut c_void) -> c_int;
    pub fn spal_csr_permute_vec_dev_f32(a: *mut spal_csr, x_dev: *const f32, y_dev: *mut f32, direction: c_int, stream: *mut c_void) -> c_int;
    pub fn spal_csc_permute_vec_f64(a: *mut spal_csc, x: *const f64, x_len: u64, y: *mut f64, y_len: u64, direction: c_int) -> c_int;
    pub fn spal_csc_permute_vec_f32(a: *mut spal_csc, x: *const f32, x_len: u64, y: *mut f32, y_len: u64, direction: c_int) -> c_int;
    pub fn spal_csc_permute_vec_dev_f64(a: *mut spal_csc, x_dev: *const f64, y_dev: *mut f64, direction: c_int, stream: *mut c_void) -> c_int;
    pub fn spal_csc_permute_vec_dev_f32(a: *mut spal_csc, x_dev: *const f32, y_dev: *mut f32, direction: c_int, stream: *mut c_void) -> c_int;
    pub fn spal_amg_default_params(params: *mut spal_amg_params) -> c_int;
    pub fn spal_amg_aggregate(n: u64, rowptr: *const u64, colind: *const u64, seed: u64, agg: *mut u64, nagg: *mut u64) -> c_int;
    pub fn spal_csr_amg_setup(a: *mut spal_csr, params: *const spal_amg_params, stream: *mut c_void, out: *mut *mut spal_amg) -> c_int;
    pub fn spal_csc_amg_setup(a: *mut spal_csc, params: *const spal_amg_params, stream: *mut c_void, out: *mut *mut spal_amg) -> c_int;
    pub fn spal_amg_destroy(g: *mut spal_amg) -> c_int;
    pub fn spal_amg_describe(g: *mut spal_amg, buf: *mut c_char, buf_len: usize) -> c_int;
    pub fn spal_amg_set_option(g: *mut spal_amg, key: *const c_char, value: i64) -> c_int;
    pub fn spal_amg_level_csr(g: *mut spal_amg, level: u64, copy: *mut *mut spal_csr) -> c_int;
    pub fn spal_amg_aggregates(g: *mut spal_amg, level: u64, agg_host: *mut u64, len: u64) -> c_int;
    pub fn spal_amg_apply_f64(g: *mut spal_amg, b: *const f64, b_len: u64, x: *mut f64, x_len: u64) -> c_int;
    pub fn spal_amg_apply_f32(g: *mut spal_amg, b: *const f32, b_len: u64, x: *mut f32, x_len: u64) -> c_int;
    pub fn spal_amg_apply_dev_f64(g: *mut spal_amg, b_dev: *const f64, x_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_amg_apply_dev_f32(g: *mut spal_amg, b_dev: *const f32, x_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_csr_krylov_amg_f64(a: *mut spal_csr, method: c_int, g: *mut spal_amg, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_amg_f32(a: *mut spal_csr, method: c_int, g: *mut spal_amg, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_amg_dev_f64(a: *mut spal_csr, method: c_int, g: *mut spal_amg, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_amg_dev_f32(a: *mut spal_csr, method: c_int, g: *mut spal_amg, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_amg_f64(a: *mut spal_csc, method: c_int, g: *mut spal_amg, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_amg_f32(a: *mut spal_csc, method: c_int, g: *mut spal_amg, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_amg_dev_f64(a: *mut spal_csc, method: c_int, g: *mut spal_amg, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_amg_dev_f32(a: *mut spal_csc, method: c_int, g: *mut spal_amg, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_fsai_setup(a: *mut spal_csr, pattern: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_fsai) -> c_int;
    pub fn spal_csc_fsai_setup(a: *mut spal_csc, pattern: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_fsai) -> c_int;
    pub fn spal_fsai_destroy(f: *mut spal_fsai) -> c_int;
    pub fn spal_fsai_describe(f: *mut spal_fsai, buf: *mut c_char, buf_len: usize) -> c_int;
    pub fn spal_fsai_factor_csr(f: *mut spal_fsai, transposed: c_int, copy: *mut *mut spal_csr) -> c_int;
    pub fn spal_fsai_apply_f64(f: *mut spal_fsai, b: *const f64, b_len: u64, x: *mut f64, x_len: u64) -> c_int;
    pub fn spal_fsai_apply_f32(f: *mut spal_fsai, b: *const f32, b_len: u64, x: *mut f32, x_len: u64) -> c_int;
    pub fn spal_fsai_apply_dev_f64(f: *mut spal_fsai, b_dev: *const f64, x_dev: *mut f64, stream: *mut c_void) -> c_int;
    pub fn spal_fsai_apply_dev_f32(f: *mut spal_fsai, b_dev: *const f32, x_dev: *mut f32, stream: *mut c_void) -> c_int;
    pub fn spal_fsai_row_f64(m: u64, b_lower: *const f64, g: *mut f64, rejected: *mut c_int) -> c_int;
    pub fn spal_fsai_row_f32(m: u64, b_lower: *const f32, g: *mut f32, rejected: *mut c_int) -> c_int;
    pub fn spal_csr_krylov_fsai_f64(a: *mut spal_csr, method: c_int, f: *mut spal_fsai, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_fsai_f32(a: *mut spal_csr, method: c_int, f: *mut spal_fsai, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_fsai_dev_f64(a: *mut spal_csr, method: c_int, f: *mut spal_fsai, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_krylov_fsai_dev_f32(a: *mut spal_csr, method: c_int, f: *mut spal_fsai, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_fsai_f64(a: *mut spal_csc, method: c_int, f: *mut spal_fsai, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_fsai_f32(a: *mut spal_csc, method: c_int, f: *mut spal_fsai, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_fsai_dev_f64(a: *mut spal_csc, method: c_int, f: *mut spal_fsai, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_krylov_fsai_dev_f32(a: *mut spal_csc, method: c_int, f: *mut spal_fsai, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_fsai_f64(a: *mut spal_csr, f: *mut spal_fsai, shift: f64, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_fsai_f32(a: *mut spal_csr, f: *mut spal_fsai, shift: f64, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_fsai_dev_f64(a: *mut spal_csr, f: *mut spal_fsai, shift: f64, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csr_minres_fsai_dev_f32(a: *mut spal_csr, f: *mut spal_fsai, shift: f64, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_fsai_f64(a: *mut spal_csc, f: *mut spal_fsai, shift: f64, b: *const f64, b_len: u64, x: *mut f64, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_fsai_f32(a: *mut spal_csc, f: *mut spal_fsai, shift: f64, b: *const f32, b_len: u64, x: *mut f32, x_len: u64, tol: f64, maxit: u64, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_fsai_dev_f64(a: *mut spal_csc, f: *mut spal_fsai, shift: f64, b_dev: *const f64, x_dev: *mut f64, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_minres_fsai_dev_f32(a: *mut spal_csc, f: *mut spal_fsai, shift: f64, b_dev: *const f32, x_dev: *mut f32, tol: f64, maxit: u64, stream: *mut c_void, info: *mut spal_krylov_info) -> c_int;
    pub fn spal_csc_to_csr(a: *mut spal_csc, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csr_to_csc(a: *mut spal_csr, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csr_mul(a: *mut spal_csr, b: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csc_mul(a: *mut spal_csc, b: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csr_add(a: *mut spal_csr, b: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csr_sub(a: *mut spal_csr, b: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csr_neg(a: *mut spal_csr, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csc_add(a: *mut spal_csc, b: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csc_sub(a: *mut spal_csc, b: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_csc_neg(a: *mut spal_csc, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_coo_upload_f64(device: c_int, nrows: u64, ncols: u64, len: u64, rows: *const u64, cols: *const u64, vals: *const f64, out: *mut *mut spal_coo) -> c_int;
    pub fn spal_coo_upload_f32(device: c_int, nrows: u64, ncols: u64, len: u64, rows: *const u64, cols: *const u64, vals: *const f32, out: *mut *mut spal_coo) -> c_int;
    pub fn spal_coo_destroy(c: *mut spal_coo) -> c_int;
    pub fn spal_coo_assemble_csr(c: *mut spal_coo, stream: *mut c_void, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_csr_plan(a: *mut spal_csr) -> c_int;
    pub fn spal_coo_assemble_csc(c: *mut spal_coo, stream: *mut c_void, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_coo_describe(c: *mut spal_coo, buf: *mut c_char, buf_len: usize) -> c_int;
    pub fn spal_coo_to_csr_f64(device: c_int, nrows: u64, ncols: u64, len: u64, rows: *const u64, cols: *const u64, vals: *const f64, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_coo_to_csr_f32(device: c_int, nrows: u64, ncols: u64, len: u64, rows: *const u64, cols: *const u64, vals: *const f32, out: *mut *mut spal_csr) -> c_int;
    pub fn spal_coo_to_csc_f64(device: c_int, nrows: u64, ncols: u64, len: u64, rows: *const u64, cols: *const u64, vals: *const f64, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_coo_to_csc_f32(device: c_int, nrows: u64, ncols: u64, len: u64, rows: *const u64, cols: *const u64, vals: *const f32, out: *mut *mut spal_csc) -> c_int;
    pub fn spal_mg_create(ngpus: c_int, devices: *const c_int, out: *mut *mut spal_mg) -> c_int;
    pub fn spal_mg_create_transport(ngpus: c_int, devices: *const c_int, transport: c_int, out: *mut *mut spal_mg) -> c_int;
    pub fn spal_mg_destroy(ctx: *mut spal_mg) -> c_int;
    pub fn spal_mg_device_count(ctx: *mut spal_mg, ngpus: *mut c_int) -> c_int;
    pub fn spal_mg_transport(ctx: *mut spal_mg, transport: *mut c_int) -> c_int;
    pub fn spal_mg_csr_create_f64(ctx: *mut spal_mg, nrows: u64, ncols: u64, rowptr: *const u64, rowptr_len: u64, colind: *const u64, colind_len: u64, values: *const f64, values_len: u64, out: *mut *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_create_f32(ctx: *mut spal_mg, nrows: u64, ncols: u64, rowptr: *const u64, rowptr_len: u64, colind: *const u64, colind_len: u64, values: *const f32, values_len: u64, out: *mut *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_destroy(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_partition(a: *mut spal_mg_csr, bounds: *mut u64) -> c_int;
    pub fn spal_mg_csr_windows(a: *mut spal_mg_csr, need_lo: *mut u64, need_hi: *mut u64) -> c_int;
    pub fn spal_mg_csr_exchange_bytes(a: *mut spal_mg_csr, x_scatter: *mut u64, y_gather: *mut u64, halo: *mut u64) -> c_int;
    pub fn spal_mg_csr_spmv_f64(a: *mut spal_mg_csr, x: *const f64, x_len: u64, y: *mut f64, y_len: u64) -> c_int;
    pub fn spal_mg_csr_spmv_f32(a: *mut spal_mg_csr, x: *const f32, x_len: u64, y: *mut f32, y_len: u64) -> c_int;
    pub fn spal_mg_csr_x_root(a: *mut spal_mg_csr, x_dev: *mut *mut c_void) -> c_int;
    pub fn spal_mg_csr_broadcast_x(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_scatter_x(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_spmv_local(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_gather_y(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_y_gathered(a: *mut spal_mg_csr, y_dev: *mut *mut c_void) -> c_int;
    pub fn spal_mg_csr_spmv_halo(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_spmv_resident(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_y_root(a: *mut spal_mg_csr, y_dev: *mut *mut c_void, slice_stride: *mut u64) -> c_int;
    pub fn spal_mg_csr_synchronize(a: *mut spal_mg_csr) -> c_int;
    pub fn spal_mg_csr_timing(a: *mut spal_mg_csr, ms: *mut f64) -> c_int;
    pub fn spal_dev_malloc(device: c_int, bytes: usize, ptr: *mut *mut c_void) -> c_int;
    pub fn spal_dev_free(device: c_int, ptr: *mut c_void) -> c_int;
    pub fn spal_memcpy_h2d(device: c_int, dst_dev: *mut c_void, src_host: *const c_void, bytes: usize) -> c_int;
    pub fn spal_memcpy_d2h(device: c_int, dst_host: *mut c_void, src_dev: *const c_void, bytes: usize) -> c_int;
    pub fn spal_device_synchronize(device: c_int) -> c_int;
    pub fn spal_cache_trim() -> c_int;
}

/// The reference panics on contract violations (`assert!`, src/csr.rs:144-156; `assert_eq!`,
/// src/csr/ops/mul.rs:9); every non-zero status keeps that convention.
pub fn check(status: c_int) {
    if status != SPAL_OK {
        let msg = unsafe { std::ffi::CStr::from_ptr(spal_last_error()) }.to_string_lossy().into_owned();
        panic!("spal_hip status {}: {}", status, msg);
    }
}

//! The operator and conversion impls the reference lacks for dense vectors (its only route to `A * x` is
//! `&a * &x_as_matrix`, src/csr/ops/mul.rs:5-59), over the device handles of `device.rs`.
use std::ops::{Add, Mul, Neg, Sub};

use super::device::{DeviceCoo, DeviceCsc, DeviceCsr};
use super::scalar::HipScalar;
use crate::{CooMatrix, CscMatrix, CsrMatrix};

/// y = A * x on the resident matrix: the form to use when a matrix multiplies more than once.
impl<T: HipScalar> Mul<&[T]> for &DeviceCsr<T> {
    type Output = Vec<T>;
    fn mul(self, x: &[T]) -> Vec<T> { self.mul_vec(x) }
}
impl<T: HipScalar> Mul<&[T]> for &DeviceCsc<T> {
    type Output = Vec<T>;
    fn mul(self, x: &[T]) -> Vec<T> { self.mul_vec(x) }
}

/// C = A * B between resident matrices: the reference's own operator (src/csr/ops/mul.rs:5-59,
/// src/csc/ops/mul.rs:5-60) on the device, bit-identical.  Panics when `a.ncols() != b.nrows()` (mul.rs:9).
impl<T: HipScalar> Mul for &DeviceCsr<T> {
    type Output = DeviceCsr<T>;
    fn mul(self, rhs: &DeviceCsr<T>) -> DeviceCsr<T> { self.mul_mat(rhs, std::ptr::null_mut()) }
}
impl<T: HipScalar> Mul for &DeviceCsc<T> {
    type Output = DeviceCsc<T>;
    fn mul(self, rhs: &DeviceCsc<T>) -> DeviceCsc<T> { self.mul_mat(rhs, std::ptr::null_mut()) }
}

/// C = A + B, A - B, -A between resident matrices: the reference's operators (src/csr/ops/{add,sub,neg}.rs,
/// src/csc/ops/{add,sub,neg}.rs) on the device, bit-identical.  Panic when the shapes differ (add.rs:9-10).
impl<T: HipScalar> Add for &DeviceCsr<T> {
    type Output = DeviceCsr<T>;
    fn add(self, rhs: &DeviceCsr<T>) -> DeviceCsr<T> { self.add_mat(rhs, std::ptr::null_mut()) }
}
impl<T: HipScalar> Sub for &DeviceCsr<T> {
    type Output = DeviceCsr<T>;
    fn sub(self, rhs: &DeviceCsr<T>) -> DeviceCsr<T> { self.sub_mat(rhs, std::ptr::null_mut()) }
}
impl<T: HipScalar> Neg for &DeviceCsr<T> {
    type Output = DeviceCsr<T>;
    fn neg(self) -> DeviceCsr<T> { self.neg_mat(std::ptr::null_mut()) }
}
impl<T: HipScalar> Add for &DeviceCsc<T> {
    type Output = DeviceCsc<T>;
    fn add(self, rhs: &DeviceCsc<T>) -> DeviceCsc<T> { self.add_mat(rhs, std::ptr::null_mut()) }
}
impl<T: HipScalar> Sub for &DeviceCsc<T> {
    type Output = DeviceCsc<T>;
    fn sub(self, rhs: &DeviceCsc<T>) -> DeviceCsc<T> { self.sub_mat(rhs, std::ptr::null_mut()) }
}
impl<T: HipScalar> Neg for &DeviceCsc<T> {
    type Output = DeviceCsc<T>;
    fn neg(self) -> DeviceCsc<T> { self.neg_mat(std::ptr::null_mut()) }
}

/// One-shot convenience with the reference's operator shape: uploads `self`, multiplies, frees the device copy.
/// The upload dominates (1.7 GB for 140M entries); keep a `DeviceCsr` (`DeviceCsr::from(&a)`) for repeated
/// products.  Panics when `x.len() != ncols` (src/csr/ops/mul.rs:9).
impl<T: HipScalar> Mul<&[T]> for &CsrMatrix<T> {
    type Output = Vec<T>;
    fn mul(self, x: &[T]) -> Vec<T> {
        assert_eq!(self.ncols(), x.len());
        DeviceCsr::new(self, 0).mul_vec(x)
    }
}
impl<T: HipScalar> Mul<&[T]> for &CscMatrix<T> {
    type Output = Vec<T>;
    fn mul(self, x: &[T]) -> Vec<T> {
        assert_eq!(self.ncols(), x.len());
        DeviceCsc::new(self, 0).mul_vec(x)
    }
}

impl<T: HipScalar> From<&CsrMatrix<T>> for DeviceCsr<T> {
    fn from(a: &CsrMatrix<T>) -> Self { DeviceCsr::new(a, 0) }
}
impl<T: HipScalar> From<&CscMatrix<T>> for DeviceCsc<T> {
    fn from(a: &CscMatrix<T>) -> Self { DeviceCsc::new(a, 0) }
}
/// `CsrMatrix::from(&coo)` on the device (src/csr/conv/coo.rs:3): upload, assemble, the COO copy is freed.
impl<T: HipScalar> From<&CooMatrix<T>> for DeviceCsr<T> {
    fn from(coo: &CooMatrix<T>) -> Self { DeviceCoo::new(coo, 0).assemble_csr() }
}
/// `CscMatrix::from(&coo)` on the device (src/csc/conv/coo.rs:3).
impl<T: HipScalar> From<&CooMatrix<T>> for DeviceCsc<T> {
    fn from(coo: &CooMatrix<T>) -> Self { DeviceCoo::new(coo, 0).assemble_csc() }
}
/// `CsrMatrix::from(&csc)` (src/csr/conv/csc.rs:4) and `CscMatrix::from(&csr)` (src/csc/conv/csr.rs:4) between
/// resident matrices: a stable sort by the minor index on the device.
impl<T: HipScalar> From<&DeviceCsc<T>> for DeviceCsr<T> {
    fn from(a: &DeviceCsc<T>) -> Self { a.to_csr() }
}
impl<T: HipScalar> From<&DeviceCsr<T>> for DeviceCsc<T> {
    fn from(a: &DeviceCsr<T>) -> Self { a.to_csc() }
}

/// Host results with the reference's own conversion signatures, computed on the device:
/// `csr_from_coo_hip(&coo)` == `CsrMatrix::from(&coo)` bit for bit.
pub fn csr_from_coo_hip<T: HipScalar>(coo: &CooMatrix<T>) -> CsrMatrix<T> { DeviceCsr::from(coo).download() }
pub fn csc_from_coo_hip<T: HipScalar>(coo: &CooMatrix<T>) -> CscMatrix<T> { DeviceCsc::from(coo).download() }
pub fn csr_from_csc_hip<T: HipScalar>(a: &CscMatrix<T>) -> CsrMatrix<T> { DeviceCsc::new(a, 0).to_csr().download() }
pub fn csc_from_csr_hip<T: HipScalar>(a: &CsrMatrix<T>) -> CscMatrix<T> { DeviceCsr::new(a, 0).to_csc().download() }
/// `&a * &b` with the reference's signatures (src/csr/ops/mul.rs:5, src/csc/ops/mul.rs:5), computed on the device.
pub fn csr_mul_hip<T: HipScalar>(a: &CsrMatrix<T>, b: &CsrMatrix<T>) -> CsrMatrix<T> {
    assert_eq!(a.ncols(), b.nrows());
    (&DeviceCsr::new(a, 0) * &DeviceCsr::new(b, 0)).download()
}
pub fn csc_mul_hip<T: HipScalar>(a: &CscMatrix<T>, b: &CscMatrix<T>) -> CscMatrix<T> {
    assert_eq!(a.ncols(), b.nrows());
    (&DeviceCsc::new(a, 0) * &DeviceCsc::new(b, 0)).download()
}
/// `&a + &b`, `&a - &b`, `-&a` with the reference's signatures (src/csr/ops/{add,sub,neg}.rs,
/// src/csc/ops/{add,sub,neg}.rs), computed on the device.
pub fn csr_add_hip<T: HipScalar>(a: &CsrMatrix<T>, b: &CsrMatrix<T>) -> CsrMatrix<T> {
    assert_eq!(a.nrows(), b.nrows());
    assert_eq!(a.ncols(), b.ncols());
    (&DeviceCsr::new(a, 0) + &DeviceCsr::new(b, 0)).download()
}
pub fn csr_sub_hip<T: HipScalar>(a: &CsrMatrix<T>, b: &CsrMatrix<T>) -> CsrMatrix<T> {
    assert_eq!(a.nrows(), b.nrows());
    assert_eq!(a.ncols(), b.ncols());
    (&DeviceCsr::new(a, 0) - &DeviceCsr::new(b, 0)).download()
}
pub fn csr_neg_hip<T: HipScalar>(a: &CsrMatrix<T>) -> CsrMatrix<T> { (-&DeviceCsr::new(a, 0)).download() }
pub fn csc_add_hip<T: HipScalar>(a: &CscMatrix<T>, b: &CscMatrix<T>) -> CscMatrix<T> {
    assert_eq!(a.nrows(), b.nrows());
    assert_eq!(a.ncols(), b.ncols());
    (&DeviceCsc::new(a, 0) + &DeviceCsc::new(b, 0)).download()
}
pub fn csc_sub_hip<T: HipScalar>(a: &CscMatrix<T>, b: &CscMatrix<T>) -> CscMatrix<T> {
    assert_eq!(a.nrows(), b.nrows());
    assert_eq!(a.ncols(), b.ncols());
    (&DeviceCsc::new(a, 0) - &DeviceCsc::new(b, 0)).download()
}
pub fn csc_neg_hip<T: HipScalar>(a: &CscMatrix<T>) -> CscMatrix<T> { (-&DeviceCsc::new(a, 0)).download() }

// spalinalg.hpp -- header-only C++ mirror of the reference's public matrix
// types over the C ABI of libspal_hip.so (include/spal.h).
//
// The reference is a Rust crate (lokyhark/spalinalg); there is no rustc in the
// build image, so the host side above the C ABI is written in C++ with the
// same names, argument meaning and error behaviour (paths relative to the
// reference root):
//
//   spalinalg::CsrMatrix<T>::CsrMatrix(nrows, ncols, rowptr, colind, values)
//       == CsrMatrix::new, incl. its panics           src/csr.rs:137-164
//   nrows() ncols() rowptr() colind() values() nnz()     src/csr.rs:200-289
//   a * x  (x a dense std::vector<T>)
//       == `&a * &x_as_matrix`, bound in Rust as
//          impl Mul<&[T]> for &CsrMatrix<T>              src/csr/ops/mul.rs:5-59
//   a * b  (b a CsrMatrix<T>) == impl Mul for &CsrMatrix<T>  src/csr/ops/mul.rs:5-59
//   a + b, a - b, -a          == impl Add / Sub / Neg for &CsrMatrix<T>  src/csr/ops/{add,sub,neg}.rs
//   CsrMatrix<T>::from(coo)  == CsrMatrix::from(&coo)    src/csr/conv/coo.rs:3-116
//   CscMatrix<T>, CooMatrix<T> likewise                  src/csc.rs, src/coo.rs
//   a.solve(b, method, M, x0, tol, maxit), dot(a, b)     not in the reference: CG / BiCGStab and their dot product
//                                                        (include/spal.h, spal_*_krylov_*, spal_*_krylov_block_*, spal_dot_*)
//   a.gmres(b, restart, M, x0, tol, maxit)               not in the reference: restarted GMRES (spal_*_gmres_*)
//   a.eigsh(k, which, ncv, v0, seed, tol, maxit)         not in the reference: extreme eigenpairs of a symmetric matrix (spal_*_eigsh_*)
//   a.eigsh_filtered(k, degree, ...), a.cheb_apply(x, degree, lo, hi, a0), a.gershgorin()    not in the reference: the Chebyshev filter (spal_*_eigsh_filtered_*, _cheb_apply_*, _gershgorin)
//   a.kpm_moments(degree, k, seed, ...), a.kpm_moments_dev(...)    not in the reference: Chebyshev moments for the spectral density and eigenvalue counts (spal_*_kpm_moments_*)
//   a.gmres_block(B, k, restart, M, X0, tol, maxit)      not in the reference: GMRES on k right-hand sides (spal_*_gmres_block_*)
//   a.minres(b, M, shift, x0, tol, maxit)                not in the reference: MINRES on (A - shift I) x = b, A symmetric (spal_*_minres_*)
//   a.minres_block(B, k, M, shift, X0, tol, maxit)       not in the reference: the same on k right-hand sides (spal_*_minres_block_*)
//   Fsai<T> f(a, &pattern), f.apply(v), f.solve(a, b, ...), f.minres(a, b, shift, ...), fsai_row(b_lower)
//                                                        not in the reference: the factorised sparse approximate inverse
//                                                        as a preconditioner (spal_*_fsai_setup, spal_fsai_*)
//   a.colour(seed), a.permute(perm), a.multicolour(seed), p.ordering(), p.to_order(v), p.from_order(v),
//   colour_greedy(n, rowptr, colind, seed), perm_from_colours(colours)
//                                                        not in the reference: the multicolour ordering
//                                                        (spal_*_colour, _permute, _multicolour, spal_colour_greedy)
//
// A failed `assert!` in the reference is a panic; here it is a
// spalinalg::Panic exception (the Rust shim in rust_shim/ turns the same
// statuses into panic!()).  Every other failure (no device, HIP error, out of
// memory) is a spalinalg::Error.  There is no CPU fallback.
//
// T is exactly the two `Scalar` impls: float, double (src/scalar.rs:56-57).
#pragma once

#include <algorithm>
#include <cstdint>
#include <limits>
#include <memory>
#include <stdexcept>
#include <string>
#include <tuple>
#include <type_traits>
#include <utility>
#include <vector>

#include "spal.h"

namespace spalinalg {

using usize = uint64_t;

struct Panic : std::logic_error {
    int status;
    Panic(int st, const std::string &m) : std::logic_error(m), status(st) {}
};
struct Error : std::runtime_error {
    int status;
    Error(int st, const std::string &m) : std::runtime_error(m), status(st) {}
};

namespace detail {
inline void check(int st) {
    if (st == SPAL_OK) return;
    const std::string msg = spal_last_error();
    if (st == SPAL_ERR_INVALID_ARGUMENT || st == SPAL_ERR_INVARIANT || st == SPAL_ERR_INDEX_OUT_OF_BOUNDS)
        throw Panic(st, msg);
    throw Error(st, msg);
}
template <typename T> struct Abi;
template <> struct Abi<double> {
    static constexpr auto csr_create = spal_csr_create_f64;
    static constexpr auto csr_spmv = spal_csr_spmv_f64;
    static constexpr auto csr_spmm = spal_csr_spmm_f64;
    static constexpr auto csr_trsv = spal_csr_trsv_f64;
    static constexpr auto csr_trsv_sweep = spal_csr_trsv_sweep_f64;
    static constexpr auto csr_trsm = spal_csr_trsm_f64;
    static constexpr auto csr_trsm_sweep = spal_csr_trsm_sweep_f64;
    static constexpr auto csr_krylov = spal_csr_krylov_f64;
    static constexpr auto csr_krylov_block = spal_csr_krylov_block_f64;
    static constexpr auto csr_gmres = spal_csr_gmres_f64;
    static constexpr auto csr_gmres_block = spal_csr_gmres_block_f64;
    static constexpr auto csr_minres = spal_csr_minres_f64;
    static constexpr auto csr_minres_block = spal_csr_minres_block_f64;
    static constexpr auto csr_eigsh = spal_csr_eigsh_f64;
    static constexpr auto csr_eigsh_filtered = spal_csr_eigsh_filtered_f64;
    static constexpr auto csr_cheb_apply = spal_csr_cheb_apply_f64;
    static constexpr auto csr_kpm_moments = spal_csr_kpm_moments_f64;
    static constexpr auto csr_kpm_moments_dev = spal_csr_kpm_moments_dev_f64;
    static constexpr auto csr_permute_vec = spal_csr_permute_vec_f64;
    static constexpr auto dot = spal_dot_f64;
    static constexpr auto csr_download = spal_csr_download_f64;
    static constexpr auto csc_create = spal_csc_create_f64;
    static constexpr auto csc_spmv = spal_csc_spmv_f64;
    static constexpr auto csc_spmm = spal_csc_spmm_f64;
    static constexpr auto csc_trsv = spal_csc_trsv_f64;
    static constexpr auto csc_trsv_sweep = spal_csc_trsv_sweep_f64;
    static constexpr auto csc_trsm = spal_csc_trsm_f64;
    static constexpr auto csc_trsm_sweep = spal_csc_trsm_sweep_f64;
    static constexpr auto csc_krylov = spal_csc_krylov_f64;
    static constexpr auto csc_krylov_block = spal_csc_krylov_block_f64;
    static constexpr auto csc_gmres = spal_csc_gmres_f64;
    static constexpr auto csc_gmres_block = spal_csc_gmres_block_f64;
    static constexpr auto csc_minres = spal_csc_minres_f64;
    static constexpr auto csc_minres_block = spal_csc_minres_block_f64;
    static constexpr auto csc_eigsh = spal_csc_eigsh_f64;
    static constexpr auto csc_eigsh_filtered = spal_csc_eigsh_filtered_f64;
    static constexpr auto csc_cheb_apply = spal_csc_cheb_apply_f64;
    static constexpr auto csc_kpm_moments = spal_csc_kpm_moments_f64;
    static constexpr auto csc_kpm_moments_dev = spal_csc_kpm_moments_dev_f64;
    static constexpr auto csc_permute_vec = spal_csc_permute_vec_f64;
    static constexpr auto coo_to_csr = spal_coo_to_csr_f64;
    static constexpr auto coo_to_csc = spal_coo_to_csc_f64;
    static constexpr auto csc_download = spal_csc_download_f64;
};
template <> struct Abi<float> {
    static constexpr auto csr_create = spal_csr_create_f32;
    static constexpr auto csr_spmv = spal_csr_spmv_f32;
    static constexpr auto csr_spmm = spal_csr_spmm_f32;
    static constexpr auto csr_trsv = spal_csr_trsv_f32;
    static constexpr auto csr_trsv_sweep = spal_csr_trsv_sweep_f32;
    static constexpr auto csr_trsm = spal_csr_trsm_f32;
    static constexpr auto csr_trsm_sweep = spal_csr_trsm_sweep_f32;
    static constexpr auto csr_krylov = spal_csr_krylov_f32;
    static constexpr auto csr_krylov_block = spal_csr_krylov_block_f32;
    static constexpr auto csr_gmres = spal_csr_gmres_f32;
    static constexpr auto csr_gmres_block = spal_csr_gmres_block_f32;
    static constexpr auto csr_minres = spal_csr_minres_f32;
    static constexpr auto csr_minres_block = spal_csr_minres_block_f32;
    static constexpr auto csr_eigsh = spal_csr_eigsh_f32;
    static constexpr auto csr_eigsh_filtered = spal_csr_eigsh_filtered_f32;
    static constexpr auto csr_cheb_apply = spal_csr_cheb_apply_f32;
    static constexpr auto csr_kpm_moments = spal_csr_kpm_moments_f32;
    static constexpr auto csr_kpm_moments_dev = spal_csr_kpm_moments_dev_f32;
    static constexpr auto csr_permute_vec = spal_csr_permute_vec_f32;
    static constexpr auto dot = spal_dot_f32;
    static constexpr auto csr_download = spal_csr_download_f32;
    static constexpr auto csc_create = spal_csc_create_f32;
    static constexpr auto csc_spmv = spal_csc_spmv_f32;
    static constexpr auto csc_spmm = spal_csc_spmm_f32;
    static constexpr auto csc_trsv = spal_csc_trsv_f32;
    static constexpr auto csc_trsv_sweep = spal_csc_trsv_sweep_f32;
    static constexpr auto csc_trsm = spal_csc_trsm_f32;
    static constexpr auto csc_trsm_sweep = spal_csc_trsm_sweep_f32;
    static constexpr auto csc_krylov = spal_csc_krylov_f32;
    static constexpr auto csc_krylov_block = spal_csc_krylov_block_f32;
    static constexpr auto csc_gmres = spal_csc_gmres_f32;
    static constexpr auto csc_gmres_block = spal_csc_gmres_block_f32;
    static constexpr auto csc_minres = spal_csc_minres_f32;
    static constexpr auto csc_minres_block = spal_csc_minres_block_f32;
    static constexpr auto csc_eigsh = spal_csc_eigsh_f32;
    static constexpr auto csc_eigsh_filtered = spal_csc_eigsh_filtered_f32;
    static constexpr auto csc_cheb_apply = spal_csc_cheb_apply_f32;
    static constexpr auto csc_kpm_moments = spal_csc_kpm_moments_f32;
    static constexpr auto csc_kpm_moments_dev = spal_csc_kpm_moments_dev_f32;
    static constexpr auto csc_permute_vec = spal_csc_permute_vec_f32;
    static constexpr auto coo_to_csr = spal_coo_to_csr_f32;
    static constexpr auto coo_to_csc = spal_coo_to_csc_f32;
    static constexpr auto csc_download = spal_csc_download_f32;
};
// assert_eq!(self.nrows(), rhs.nrows()); assert_eq!(self.ncols(), rhs.ncols())  (src/csr/ops/add.rs:9-10, sub.rs:9-10)
inline void check_same_shape(usize nrows, usize ncols, usize rhs_nrows, usize rhs_ncols) {
    if (nrows != rhs_nrows)
        throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: nrows == rhs.nrows (left: " + std::to_string(nrows) +
                                                   ", right: " + std::to_string(rhs_nrows) + ")");
    if (ncols != rhs_ncols)
        throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.ncols (left: " + std::to_string(ncols) +
                                                   ", right: " + std::to_string(rhs_ncols) + ")");
}
struct CsrDeleter { void operator()(spal_csr *h) const { spal_csr_destroy(h); } };
struct CscDeleter { void operator()(spal_csc *h) const { spal_csc_destroy(h); } };
}  // namespace detail

template <typename T> class CooMatrix;
template <typename T> class CscMatrix;

// The Krylov solvers of include/spal.h (spal_*_krylov_*): the method, and what a solve returns beside x.
enum class Method { Cg = SPAL_KRYLOV_CG, BiCgStab = SPAL_KRYLOV_BICGSTAB };
template <typename T>
struct Solution {
    std::vector<T> x;
    usize iterations;
    int reason;   // 0 converged (dot(r, r) <= tol^2 dot(b, b)), 1 maxit reached, 2 breakdown / not finite
    double residual_sq, rhs_sq, solve_ms;
};

// What kpm_moments returns: mu[i * probes + j] = moment i of probe column j, and the call's report (include/spal.h).
struct KpmMoments {
    std::vector<double> mu;
    spal_kpm_info info{};
};

// What eigsh returns: `pairs` eigenvalues in the order asked for (LA descending, SA ascending), their estimates
// |hn * Y[m-1, i]|, and X row-major (element (i, j) at i * pairs + j; empty when no vectors were asked for).
enum class Which : int { LA = SPAL_EIGSH_LA, SA = SPAL_EIGSH_SA };
template <typename T>
struct Eigenpairs {
    std::vector<T> theta, resid, x;
    usize pairs, restarts, products, converged;
    int reason;   // 0 converged (or the space exhausted with >= k pairs), 1 maxit restarts, 2 not finite, 3 exhausted below k
    double solve_ms;
};

// What eigsh_filtered adds to eigsh's result: resid holds TRUE residual norms; the warm-up's counts (automatic interval),
// the interval the polynomial is small on (0, 0: the warm-up's result was returned), a0 and the degree.
template <typename T>
struct FilteredEigenpairs {
    Eigenpairs<T> pairs;
    usize warm_restarts, warm_products, degree;
    double lo, hi, a0;
};

// What solve_block returns: X row-major (element (i, j) at i * k + j) and one record per column, as Solution holds one.
struct ColumnResult {
    usize iterations;
    int reason;
    double residual_sq, rhs_sq, solve_ms;   // solve_ms: the call's time, the same in every column
};
template <typename T>
struct BlockSolution {
    std::vector<T> x;
    std::vector<ColumnResult> columns;
};

// dot(a, b) by the library's definition: products rounded, then the fixed tree over tiles of 1024 (spal_dot_*, host only).
template <typename T>
T dot(const std::vector<T> &a, const std::vector<T> &b) {
    if (a.size() != b.size())
        throw Panic(SPAL_ERR_INVALID_ARGUMENT, "dot: a.len() = " + std::to_string(a.size()) + " but b.len() = " +
                                                   std::to_string(b.size()));
    T out = T(0);
    detail::check(detail::Abi<T>::dot(a.data(), b.data(), a.size(), &out));
    return out;
}

// The multicolour ordering of include/spal.h: what colour() returns, and what ordering() reads back from a
// matrix made by permute() or multicolour().
struct Colouring {
    std::vector<usize> colours;
    usize ncolours, rounds;   // rounds: Jones-Plassmann rounds = the longest path of descending keys, in vertices
};
struct Ordering {
    std::vector<usize> perm;  // new -> old
    usize ncolours;           // 0: the permutation was the caller's
};
// The text itself on host arrays, no device (spal_colour_greedy, spal_perm_from_colours): colours by descending
// key(i) = mix32(i + seed), and the rows listed by (colour, row).
inline Colouring colour_greedy(usize n, const std::vector<usize> &rowptr, const std::vector<usize> &colind, usize seed = 0) {
    if (rowptr.size() != n + 1)
        throw Panic(SPAL_ERR_INVALID_ARGUMENT, "colour_greedy: rowptr.len() = " + std::to_string(rowptr.size()) +
                                                   " but n + 1 = " + std::to_string(n + 1));
    if (colind.size() < rowptr[n])
        throw Panic(SPAL_ERR_INVALID_ARGUMENT, "colour_greedy: colind.len() = " + std::to_string(colind.size()) +
                                                   " but rowptr[n] = " + std::to_string(rowptr[n]));
    Colouring c{std::vector<usize>(n), 0, 0};
    detail::check(spal_colour_greedy(n, rowptr.data(), colind.data(), seed, c.colours.data(), &c.ncolours));
    return c;
}
inline std::vector<usize> perm_from_colours(const std::vector<usize> &colours) {
    std::vector<usize> perm(colours.size());
    detail::check(spal_perm_from_colours(colours.size(), colours.data(), perm.data()));
    return perm;
}

// ---------------------------------------------------------------------------
// CsrMatrix<T>                                     reference src/csr.rs:66-72
// ---------------------------------------------------------------------------
template <typename T>
class CsrMatrix {
    static_assert(std::is_same<T, float>::value || std::is_same<T, double>::value,
                  "Scalar is implemented for f32 and f64 only");

  public:
    // CsrMatrix::new -- panics exactly where the reference does.
    CsrMatrix(usize nrows, usize ncols, std::vector<usize> rowptr, std::vector<usize> colind,
              std::vector<T> values)
        : nrows_(nrows), ncols_(ncols), rowptr_(std::move(rowptr)), colind_(std::move(colind)),
          values_(std::move(values)) {
        int reason = 0;
        detail::check(spal_csr_validate(nrows_, ncols_, rowptr_.data(), rowptr_.size(), colind_.data(),
                                        colind_.size(), values_.size(), &reason));
    }

    usize nrows() const { return nrows_; }
    usize ncols() const { return ncols_; }
    const std::vector<usize> &rowptr() const { return rowptr_; }
    const std::vector<usize> &colind() const { return colind_; }
    const std::vector<T> &values() const { return values_; }
    usize nnz() const { return rowptr_[nrows_]; }

    // Device copy (created on first use, owned by this object).
    spal_csr_t device_handle(int device = 0) const {
        if (!dev_) {
            spal_csr_t h = nullptr;
            detail::check(detail::Abi<T>::csr_create(device, nrows_, ncols_, rowptr_.data(), rowptr_.size(),
                                                     colind_.data(), colind_.size(), values_.data(),
                                                     values_.size(), &h));
            dev_.reset(h);
        }
        return dev_.get();
    }

    // y = A * x.  Panics when x.len() != ncols (assert_eq!, src/csr/ops/mul.rs:9).
    std::vector<T> operator*(const std::vector<T> &x) const {
        if (x.size() != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: `(left == right)` ncols vs x.len()");
        std::vector<T> y(nrows_);
        detail::check(detail::Abi<T>::csr_spmv(device_handle(), x.data(), x.size(), y.data(), y.size()));
        return y;
    }

    // Y = A * X for a dense ROW-MAJOR block of k vectors (x.size() == ncols * k, element (i, j) at i * k + j): one pass
    // over the matrix for all k columns, bit for bit `&A * &X` with every entry of X stored.  Panics when X has another
    // number of rows than ncols (assert_eq!, src/csr/ops/mul.rs:9).  With one or two vectors operator* is the faster call.
    std::vector<T> mul(const std::vector<T> &x, usize k) const {
        if (k == 0 || x.size() % k != 0 || x.size() / k != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.nrows (left: " + std::to_string(ncols_) +
                                                       ", right: " + std::to_string(k ? x.size() / k : 0) + ")");
        std::vector<T> y(nrows_ * k);
        detail::check(detail::Abi<T>::csr_spmm(device_handle(), k, x.data(), k, ncols_, y.data(), k, nrows_));
        return y;
    }

    // x with L x = b (the lower triangle of this matrix, `lower`) or U x = b; entries of the other triangle are ignored,
    // `unit_diagonal` takes the diagonal as ones.  Substitution on the device, bit for bit the sequential loop of
    // include/spal.h (spal_csr_trsv_*).  Panics when the matrix is not square, when b has another length than nrows,
    // and (without unit_diagonal) when a row stores no diagonal entry.
    std::vector<T> solve_triangular(const std::vector<T> &b, bool lower = true, bool unit_diagonal = false) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular: the matrix is not square (" + std::to_string(nrows_) +
                                                       " x " + std::to_string(ncols_) + ")");
        if (b.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular: b.len() = " + std::to_string(b.size()) +
                                                       " but the matrix has " + std::to_string(nrows_) + " rows");
        std::vector<T> x(nrows_);
        detail::check(detail::Abi<T>::csr_trsv(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, b.data(), b.size(),
                                               x.data(), x.size()));
        return x;
    }

    // `sweeps` Jacobi passes on the chosen triangle instead of the substitution (spal_csr_trsv_sweep_*, the sequential
    // text in include/spal.h, bit for bit): an approximate solve in launches whose rows are all independent; from
    // sweeps = levels - 1 on it IS solve_triangular's result.  Panics as solve_triangular does.
    std::vector<T> solve_triangular_sweeps(const std::vector<T> &b, bool lower, bool unit_diagonal, std::uint64_t sweeps) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular_sweeps: the matrix is not square (" +
                                                       std::to_string(nrows_) + " x " + std::to_string(ncols_) + ")");
        if (b.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular_sweeps: b.len() = " + std::to_string(b.size()) +
                                                       " but the matrix has " + std::to_string(nrows_) + " rows");
        std::vector<T> x(nrows_);
        detail::check(detail::Abi<T>::csr_trsv_sweep(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, sweeps, b.data(),
                                                     b.size(), x.data(), x.size()));
        return x;
    }

    // the host-side refusals of the block solves, before any device call
    void check_block(const char *who, std::size_t len, usize k) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(who) + ": the matrix is not square (" +
                                                       std::to_string(nrows_) + " x " + std::to_string(ncols_) + ")");
        if (k == 0) throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(who) + ": k = 0 (B and X need at least one column)");
        if (len % k != 0 || len / k != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(who) + ": B.len() = " + std::to_string(len) + " is not " +
                                                       std::to_string(nrows_) + " rows of k = " + std::to_string(k));
    }

    // X with L X = B / U X = B for a ROW-MAJOR block of k right-hand sides (B.size() == nrows * k, element (i, j) at
    // i * k + j): column j of the result is bit for bit solve_triangular's result for column j of B, and all k columns
    // share one solve's launches (spal_csr_trsm_*).  Panics as solve_triangular does, and when k == 0 or B has another
    // number of rows than the matrix.
    std::vector<T> solve_triangular_block(const std::vector<T> &B, usize k, bool lower = true, bool unit_diagonal = false) const {
        check_block("solve_triangular_block", B.size(), k);
        std::vector<T> x(nrows_ * k);
        detail::check(detail::Abi<T>::csr_trsm(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, k, B.data(), k,
                                               nrows_, x.data(), k, nrows_));
        return x;
    }

    // ... and by `sweeps` Jacobi passes per column (spal_csr_trsm_sweep_*): column j is solve_triangular_sweeps' result
    // for column j of B; a pass stages the matrix once for all k columns.
    std::vector<T> solve_triangular_block_sweeps(const std::vector<T> &B, usize k, bool lower, bool unit_diagonal,
                                                 std::uint64_t sweeps) const {
        check_block("solve_triangular_block_sweeps", B.size(), k);
        std::vector<T> x(nrows_ * k);
        detail::check(detail::Abi<T>::csr_trsm_sweep(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, sweeps, k,
                                                     B.data(), k, nrows_, x.data(), k, nrows_));
        return x;
    }

    // C = A * B: `impl Mul for &CsrMatrix<T>` (src/csr/ops/mul.rs:5-59) on the device, bit-identical.
    // Panics when ncols != rhs.nrows (assert_eq!, mul.rs:9).
    CsrMatrix operator*(const CsrMatrix &rhs) const {
        if (ncols_ != rhs.nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.nrows (left: " +
                                                       std::to_string(ncols_) + ", right: " + std::to_string(rhs.nrows_) + ")");
        spal_csr_t h = nullptr;
        detail::check(spal_csr_mul(device_handle(), rhs.device_handle(), nullptr, &h));
        return adopt(h);
    }

    // C = A + B / A - B / -A: `impl Add / Sub / Neg for &CsrMatrix<T>` (src/csr/ops/{add,sub,neg}.rs) on the device,
    // bit-identical.  Panics when the shapes differ (assert_eq!, add.rs:9-10 / sub.rs:9-10), before any device call.
    CsrMatrix operator+(const CsrMatrix &rhs) const { return add_sub(rhs, spal_csr_add); }
    CsrMatrix operator-(const CsrMatrix &rhs) const { return add_sub(rhs, spal_csr_sub); }
    CsrMatrix operator-() const {
        spal_csr_t h = nullptr;
        detail::check(spal_csr_neg(device_handle(), nullptr, &h));
        return adopt(h);
    }

    // The ILU(0) factor of this square matrix (spal_csr_ilu0, include/spal.h): the same structure, L strictly below the
    // diagonal with its unit diagonal implied, U on and above it, bit for bit the sequential loop without fill.
    // M^-1 r is f.solve_triangular(f.solve_triangular(r, true, true), false).  Panics when the matrix is not square or
    // a row stores no diagonal entry.
    CsrMatrix ilu0() const {
        spal_csr_t h = nullptr;
        detail::check(spal_csr_ilu0(device_handle(), nullptr, &h));
        return adopt(h);
    }
    // ILU(0) by `sweeps` row sweeps (spal_csr_ilu0_sweep, include/spal.h): every pass factorises every row on its own
    // against the previous pass's factor -- no analysis, one SpMV-shaped launch per pass, bit for bit the sequential
    // text, and ilu0()'s bits from sweeps = levels - 1 on.  Meant to be applied by sweeps too (option "trsv_sweeps").
    CsrMatrix ilu0(uint64_t sweeps) const {
        if (nrows_ != ncols_)   // before any device call
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "ilu0: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        spal_csr_t h = nullptr;
        detail::check(spal_csr_ilu0_sweep(device_handle(), sweeps, nullptr, &h));
        return adopt(h);
    }

    // The multicolour ordering (include/spal.h).  colour(): the greedy colouring of the graph of A + A^T by
    // hashed priority, exactly the sequential text, by rounds on the device.  permute(perm): B = P A P^T with
    // B[i'][j'] = A[perm[i']][perm[j']], values moved.  multicolour(): the rows numbered colour by colour, so that both
    // triangles (and those of ilu0()) have at most ncolours levels.  The results keep their permutation: ordering()
    // reads it back, to_order(v) = v[perm] and from_order() its inverse move a vector between the two numberings:
    //   auto p = a.multicolour(); auto f = p.ilu0();
    //   auto x = p.from_order(p.solve(p.to_order(b), Method::BiCgStab, &f).x);
    // Panic when the matrix is not square, perm is no permutation, or (ordering, to_order, from_order) the matrix is no
    // result of permute() / multicolour().
    Colouring colour(usize seed = 0) const {
        Colouring c{std::vector<usize>(nrows_), 0, 0};
        detail::check(spal_csr_colour(device_handle(), seed, nullptr, c.colours.data(), &c.ncolours, &c.rounds));
        return c;
    }
    CsrMatrix permute(const std::vector<usize> &perm) const {
        spal_csr_t h = nullptr;
        detail::check(spal_csr_permute(device_handle(), perm.data(), perm.size(), nullptr, &h));
        return adopt(h);
    }
    CsrMatrix multicolour(usize seed = 0) const {
        spal_csr_t h = nullptr;
        usize ncolours = 0;
        detail::check(spal_csr_multicolour(device_handle(), seed, nullptr, &h, &ncolours));
        return adopt(h);
    }
    Ordering ordering() const {
        Ordering o{std::vector<usize>(nrows_), 0};
        detail::check(spal_csr_ordering(device_handle(), o.perm.data(), &o.ncolours));
        return o;
    }
    std::vector<T> to_order(const std::vector<T> &v) const { return permute_vec(v, 0); }
    std::vector<T> from_order(const std::vector<T> &v) const { return permute_vec(v, 1); }

    // x with A x = b by CG (A symmetric positive definite) or BiCGStab on the device, optionally preconditioned by
    // M = ilu0() (nullptr: none), from x0 (empty: zeros); bit for bit the loops of include/spal.h (spal_csr_krylov_*).
    // Panics when the matrix is not square or a length differs; a breakdown is no panic but reason 2.
    Solution<T> solve(const std::vector<T> &b, Method method = Method::Cg, const CsrMatrix *M = nullptr,
                      const std::vector<T> &x0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve: b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        Solution<T> s{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
        spal_krylov_info info;
        detail::check(detail::Abi<T>::csr_krylov(device_handle(), static_cast<int>(method), M ? M->device_handle() : nullptr,
                                                  b.data(), b.size(), s.x.data(), s.x.size(), tol, maxit, &info));
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }

    // X with A X = B for a ROW-MAJOR block of k right-hand sides (B.size() == nrows * k): k independent CG / BiCGStab
    // iterations in lockstep on shared launches (spal_csr_krylov_block_*, include/spal.h).  Column j of the result and
    // columns[j] are bit for bit solve()'s loop on column j of B, whatever k and the other columns are; a column that has
    // stopped is frozen while the others run on.  X0 empty: zeros.  Panics as solve() does, and when k == 0 or B / X0
    // are not nrows x k.
    BlockSolution<T> solve_block(const std::vector<T> &B, usize k, Method method = Method::Cg, const CsrMatrix *M = nullptr,
                                 const std::vector<T> &X0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        check_block("solve_block", B.size(), k);
        if (!X0.empty() && X0.size() != B.size())
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_block: X0.len() = " + std::to_string(X0.size()) +
                                                       " but B.len() = " + std::to_string(B.size()));
        BlockSolution<T> s{X0.empty() ? std::vector<T>(B.size(), T(0)) : X0, {}};
        std::vector<spal_krylov_info> info(k);
        detail::check(detail::Abi<T>::csr_krylov_block(device_handle(), static_cast<int>(method),
                                                        M ? M->device_handle() : nullptr, k, B.data(), k, nrows_,
                                                        s.x.data(), k, nrows_, tol, maxit, info.data()));
        for (const spal_krylov_info &c : info)
            s.columns.push_back(ColumnResult{c.iterations, c.reason, c.residual_sq, c.rhs_sq, c.solve_ms});
        return s;
    }

    // x with A x = b by restarted GMRES(restart) on the device, for matrices that are not symmetric; right-preconditioned
    // by M as solve() is; bit for bit the text of include/spal.h (spal_csr_gmres_*).  restart is 1 .. 256.  Reasons 0 and
    // 1 are decided on the true residual.  Panics as solve() does, and on a restart outside its range.
    Solution<T> gmres(const std::vector<T> &b, usize restart = 30, const CsrMatrix *M = nullptr,
                      const std::vector<T> &x0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres: b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        if (restart == 0 || restart > 256)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres: restart = " + std::to_string(restart) + " must be 1 .. 256");
        Solution<T> s{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
        spal_krylov_info info;
        detail::check(detail::Abi<T>::csr_gmres(device_handle(), M ? M->device_handle() : nullptr, b.data(), b.size(),
                                                 s.x.data(), s.x.size(), restart, tol, maxit, &info));
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }

    // The k largest (Which::LA) or smallest (Which::SA) eigenpairs of this SYMMETRIC matrix (not checked) by thick-restart
    // Lanczos with full orthogonalisation on the device; bit for bit the text of include/spal.h (spal_csr_eigsh_*).  ncv = 0:
    // min(n, max(2k + 1, 20)); tol = 0: the element type's machine epsilon; v0 empty: the text's start vector from `seed`.
    // An eigenvalue of multiplicity > 1 is returned ONCE.  Panics on a matrix that is not square, k == 0, ncv <= k,
    // ncv > 256 or ncv > n.
    Eigenpairs<T> eigsh(usize k = 6, Which which = Which::LA, usize ncv = 0, const std::vector<T> &v0 = {}, usize seed = 0,
                        double tol = 0.0, usize maxit = 1000, bool vectors = true) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (ncv == 0) ncv = std::min<usize>(nrows_, std::max<usize>(2 * k + 1, 20));
        if (k == 0 || ncv <= k || ncv > 256 || ncv > nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh: k = " + std::to_string(k) + " and ncv = " + std::to_string(ncv) +
                                                       " must satisfy 0 < k < ncv <= min(256, " + std::to_string(nrows_) + ")");
        if (!v0.empty() && v0.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh: v0.len() = " + std::to_string(v0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        if (tol == 0.0) tol = static_cast<double>(std::numeric_limits<T>::epsilon());
        Eigenpairs<T> e{std::vector<T>(k, T(0)), std::vector<T>(k, T(0)), std::vector<T>(vectors ? nrows_ * k : 0, T(0)), 0, 0, 0, 0, 0, 0.0};
        spal_eigsh_info info;
        detail::check(detail::Abi<T>::csr_eigsh(device_handle(), k, static_cast<int>(which), ncv, v0.empty() ? nullptr : v0.data(),
                                                 v0.size(), seed, tol, maxit, e.theta.data(), k, e.resid.data(), k,
                                                 vectors ? e.x.data() : nullptr, k, nrows_, &info));
        e.pairs = info.reason == 2 ? 0 : info.reason == 3 ? info.converged : k;
        e.restarts = info.restarts;
        e.products = info.products;
        e.converged = info.converged;
        e.reason = info.reason;
        e.solve_ms = info.solve_ms;
        if (e.pairs < k) {   // pack the columns that were written
            std::vector<T> x(vectors ? nrows_ * e.pairs : 0);
            for (usize i = 0; vectors && i < nrows_; ++i)
                for (usize j = 0; j < e.pairs; ++j) x[i * e.pairs + j] = e.x[i * k + j];
            e.x.swap(x);
            e.theta.resize(e.pairs);
            e.resid.resize(e.pairs);
        }
        return e;
    }

    // eigsh on a Chebyshev polynomial of A of `degree` (1 .. 256), for CLUSTERED extreme eigenvalues (spal_csr_eigsh_filtered_*,
    // include/spal.h): automatic = true takes the interval to damp from `warmup` restarts of eigsh's own iteration, false
    // uses [lo, hi].  Convergence is decided on true residuals against tol * max(|glo|, |ghi|); tol = 0: 256 epsilons.
    FilteredEigenpairs<T> eigsh_filtered(usize k, usize degree, Which which = Which::LA, usize ncv = 0, bool automatic = true,
                                         double lo = 0.0, double hi = 0.0, usize warmup = 5, const std::vector<T> &v0 = {},
                                         usize seed = 0, double tol = 0.0, usize maxit = 1000, bool vectors = true) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (ncv == 0) ncv = std::min<usize>(nrows_, std::max<usize>(2 * k + 1, 20));
        if (k == 0 || ncv <= k || ncv > 256 || ncv > nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: k = " + std::to_string(k) + " and ncv = " + std::to_string(ncv) +
                                                       " must satisfy 0 < k < ncv <= min(256, " + std::to_string(nrows_) + ")");
        if (degree < 1 || degree > 256)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: degree = " + std::to_string(degree) + " must be 1 .. 256");
        if (!v0.empty() && v0.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: v0.len() = " + std::to_string(v0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        FilteredEigenpairs<T> f{{std::vector<T>(k, T(0)), std::vector<T>(k, T(0)), std::vector<T>(vectors ? nrows_ * k : 0, T(0)), 0, 0, 0, 0, 0, 0.0},
                                0, 0, degree, 0.0, 0.0, 0.0};
        Eigenpairs<T> &e = f.pairs;
        spal_eigsh_filter_info info;
        detail::check(detail::Abi<T>::csr_eigsh_filtered(device_handle(), k, static_cast<int>(which), ncv, v0.empty() ? nullptr : v0.data(),
                                                          v0.size(), seed, tol, maxit, degree, automatic ? 1 : 0, lo, hi, warmup,
                                                          e.theta.data(), k, e.resid.data(), k, vectors ? e.x.data() : nullptr, k,
                                                          nrows_, &info));
        e.pairs = info.reason == 2 ? 0 : info.reason == 3 ? info.converged : k;
        e.restarts = info.restarts;
        e.products = info.products;
        e.converged = info.converged;
        e.reason = info.reason;
        e.solve_ms = info.solve_ms;
        f.warm_restarts = info.warm_restarts;
        f.warm_products = info.warm_products;
        f.lo = info.lo;
        f.hi = info.hi;
        f.a0 = info.a0;
        if (e.pairs < k) {   // pack the columns that were written
            std::vector<T> x(vectors ? nrows_ * e.pairs : 0);
            for (usize i = 0; vectors && i < nrows_; ++i)
                for (usize j = 0; j < e.pairs; ++j) x[i * e.pairs + j] = e.x[i * k + j];
            e.x.swap(x);
            e.theta.resize(e.pairs);
            e.resid.resize(e.pairs);
        }
        return f;
    }

    // t_d = p(A) x: the Chebyshev polynomial of `degree` that is small on [lo, hi] and 1 at a0, outside the interval
    // (spal_csr_cheb_apply_*): the text of include/spal.h bit for bit.  Panics as the library refuses.
    std::vector<T> cheb_apply(const std::vector<T> &x, usize degree, double lo, double hi, double a0) const {
        std::vector<T> out(nrows_, T(0));
        detail::check(detail::Abi<T>::csr_cheb_apply(device_handle(), x.data(), x.size(), out.data(), out.size(), degree, lo, hi, a0));
        return out;
    }

    // (glo, ghi): Gershgorin's enclosure of the spectrum, in double (spal_csr_gershgorin)
    std::pair<double, double> gershgorin() const {
        double lo = 0.0, hi = 0.0;
        detail::check(spal_csr_gershgorin(device_handle(), &lo, &hi));
        return {lo, hi};
    }

    // The KPM moments mu[i * k + j] = z_j^T T_i(B) z_j, i = 0 .. degree, of k probe columns (spal_csr_kpm_moments_*,
    // include/spal.h): the text bit for bit, in double.  z empty: hashed +-1 probes from `seed`, else a ROW-MAJOR
    // nrows x k block.  automatic: Gershgorin's bounds with a margin, else [lo, hi], which must enclose the spectrum.
    // The matrix must be symmetric (not checked).  Panics as the library refuses.
    KpmMoments kpm_moments(usize degree, usize k = 8, usize seed = 0, bool automatic = true, double lo = 0.0, double hi = 0.0,
                           const std::vector<T> &z = {}) const {
        KpmMoments out;
        out.mu.assign((degree + 1) * k, 0.0);
        detail::check(detail::Abi<T>::csr_kpm_moments(device_handle(), degree, k, seed, automatic ? 1 : 0, lo, hi,
                                                      z.empty() ? nullptr : z.data(), k ? z.size() / k : 0, k, out.mu.data(),
                                                      out.mu.size(), &out.info));
        return out;
    }
    // ... with the probes in device memory (z_dev == nullptr: hashed), enqueued on `stream`; synchronises once, at its end
    KpmMoments kpm_moments_dev(usize degree, usize k, usize seed, bool automatic, double lo, double hi, const T *z_dev, usize ldz,
                               void *stream) const {
        KpmMoments out;
        out.mu.assign((degree + 1) * k, 0.0);
        detail::check(detail::Abi<T>::csr_kpm_moments_dev(device_handle(), degree, k, seed, automatic ? 1 : 0, lo, hi, z_dev, ldz,
                                                          out.mu.data(), out.mu.size(), stream, &out.info));
        return out;
    }

    // X with A X = B for a ROW-MAJOR block of k right-hand sides by restarted GMRES(restart): k independent iterations in
    // lockstep on shared launches, with cycles common to the block (spal_csr_gmres_block_*, include/spal.h).  Column j
    // of the result and columns[j] are bit for bit gmres()'s text on column j of B, whatever k and the other columns are.
    // X0 empty: zeros.  Panics as gmres() does, and when k == 0 or B / X0 are not nrows x k.
    BlockSolution<T> gmres_block(const std::vector<T> &B, usize k, usize restart = 30, const CsrMatrix *M = nullptr,
                                 const std::vector<T> &X0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        check_block("gmres_block", B.size(), k);
        if (!X0.empty() && X0.size() != B.size())
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres_block: X0.len() = " + std::to_string(X0.size()) +
                                                       " but B.len() = " + std::to_string(B.size()));
        if (restart == 0 || restart > 256)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres_block: restart = " + std::to_string(restart) + " must be 1 .. 256");
        BlockSolution<T> s{X0.empty() ? std::vector<T>(B.size(), T(0)) : X0, {}};
        std::vector<spal_krylov_info> info(k);
        detail::check(detail::Abi<T>::csr_gmres_block(device_handle(), M ? M->device_handle() : nullptr, k, B.data(), k,
                                                       nrows_, s.x.data(), k, nrows_, restart, tol, maxit, info.data()));
        for (const spal_krylov_info &c : info)
            s.columns.push_back(ColumnResult{c.iterations, c.reason, c.residual_sq, c.rhs_sq, c.solve_ms});
        return s;
    }

    // x with (A - shift I) x = b by MINRES on the device, for a SYMMETRIC matrix that may be indefinite (not checked); M,
    // when given, symmetric positive definite and applied as solve() applies it; bit for bit the text of include/spal.h
    // (spal_csr_minres_*).  The residual estimate never grows, so reason 1 still returns the best iterate.  Panics as
    // solve() does, and on a shift that is not finite.
    Solution<T> minres(const std::vector<T> &b, const CsrMatrix *M = nullptr, double shift = 0.0, const std::vector<T> &x0 = {},
                       double tol = 1e-8, usize maxit = 1000) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres: b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        if (!(shift - shift == 0.0)) throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres: shift must be finite");
        Solution<T> s{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
        spal_krylov_info info;
        detail::check(detail::Abi<T>::csr_minres(device_handle(), M ? M->device_handle() : nullptr, shift, b.data(),
                                                  b.size(), s.x.data(), s.x.size(), tol, maxit, &info));
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }

    // X with (A - shift I) X = B for a ROW-MAJOR block of k right-hand sides by MINRES: k independent iterations in
    // lockstep on shared launches (spal_csr_minres_block_*, include/spal.h).  Column j of the result and columns[j] are
    // bit for bit minres()'s text on column j of B, whatever k and the other columns are.  X0 empty: zeros.  Panics as
    // minres() does, and when k == 0 or B / X0 are not nrows x k.
    BlockSolution<T> minres_block(const std::vector<T> &B, usize k, const CsrMatrix *M = nullptr, double shift = 0.0,
                                  const std::vector<T> &X0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        check_block("minres_block", B.size(), k);
        if (!X0.empty() && X0.size() != B.size())
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres_block: X0.len() = " + std::to_string(X0.size()) +
                                                       " but B.len() = " + std::to_string(B.size()));
        if (!(shift - shift == 0.0)) throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres_block: shift must be finite");
        BlockSolution<T> s{X0.empty() ? std::vector<T>(B.size(), T(0)) : X0, {}};
        std::vector<spal_krylov_info> info(k);
        detail::check(detail::Abi<T>::csr_minres_block(device_handle(), M ? M->device_handle() : nullptr, shift, k, B.data(),
                                                        k, nrows_, s.x.data(), k, nrows_, tol, maxit, info.data()));
        for (const spal_krylov_info &c : info)
            s.columns.push_back(ColumnResult{c.iterations, c.reason, c.residual_sq, c.rhs_sq, c.solve_ms});
        return s;
    }

    // CsrMatrix::from(&coo): assembled on the device, bit-identical to the reference.
    static CsrMatrix from(const CooMatrix<T> &coo, int device = 0);
    // CsrMatrix::from(&csc)  (src/csr/conv/csc.rs:4-52): device stable sort by row.
    static CsrMatrix from(const CscMatrix<T> &csc, int device = 0);

  private:
    friend class CscMatrix<T>;
    struct Trusted {};
    CsrMatrix(Trusted, usize nrows, usize ncols, std::vector<usize> rp, std::vector<usize> ci,
              std::vector<T> va)
        : nrows_(nrows), ncols_(ncols), rowptr_(std::move(rp)), colind_(std::move(ci)),
          values_(std::move(va)) {}
    CsrMatrix add_sub(const CsrMatrix &rhs, int (*op)(spal_csr_t, spal_csr_t, void *, spal_csr_t *)) const {
        detail::check_same_shape(nrows_, ncols_, rhs.nrows_, rhs.ncols_);
        spal_csr_t h = nullptr;
        detail::check(op(device_handle(), rhs.device_handle(), nullptr, &h));
        return adopt(h);
    }
    std::vector<T> permute_vec(const std::vector<T> &v, int direction) const {
        std::vector<T> y(v.size());
        detail::check(detail::Abi<T>::csr_permute_vec(device_handle(), v.data(), v.size(), y.data(), y.size(), direction));
        return y;
    }
    static CsrMatrix adopt(spal_csr_t h) {   // downloads h into a host matrix that also owns h
        std::unique_ptr<spal_csr, detail::CsrDeleter> guard(h);
        uint64_t nr = 0, nc = 0, nz = 0;
        int es = 0;
        detail::check(spal_csr_shape(h, &nr, &nc, &nz, &es));
        std::vector<usize> rp(nr + 1), ci(nz);
        std::vector<T> va(nz);
        detail::check(detail::Abi<T>::csr_download(h, rp.data(), ci.data(), va.data()));
        // struct-literal construction like the reference (src/csr/conv/coo.rs:108-114)
        CsrMatrix out(Trusted{}, nr, nc, std::move(rp), std::move(ci), std::move(va));
        out.dev_ = std::move(guard);
        return out;
    }
    usize nrows_, ncols_;
    std::vector<usize> rowptr_, colind_;
    std::vector<T> values_;
    mutable std::unique_ptr<spal_csr, detail::CsrDeleter> dev_;
};

// ---------------------------------------------------------------------------
// CscMatrix<T>                                     reference src/csc.rs:66-72
// ---------------------------------------------------------------------------
template <typename T>
class CscMatrix {
  public:
    CscMatrix(usize nrows, usize ncols, std::vector<usize> colptr, std::vector<usize> rowind,
              std::vector<T> values)
        : nrows_(nrows), ncols_(ncols), colptr_(std::move(colptr)), rowind_(std::move(rowind)),
          values_(std::move(values)) {
        int reason = 0;
        detail::check(spal_csc_validate(nrows_, ncols_, colptr_.data(), colptr_.size(), rowind_.data(),
                                        rowind_.size(), values_.size(), &reason));
    }
    usize nrows() const { return nrows_; }
    usize ncols() const { return ncols_; }
    const std::vector<usize> &colptr() const { return colptr_; }
    const std::vector<usize> &rowind() const { return rowind_; }
    const std::vector<T> &values() const { return values_; }
    usize nnz() const { return colptr_[ncols_]; }

    spal_csc_t device_handle(int device = 0) const {
        if (!dev_) {
            spal_csc_t h = nullptr;
            detail::check(detail::Abi<T>::csc_create(device, nrows_, ncols_, colptr_.data(), colptr_.size(),
                                                     rowind_.data(), rowind_.size(), values_.data(),
                                                     values_.size(), &h));
            dev_.reset(h);
        }
        return dev_.get();
    }
    // y = A * x; panics when x.len() != ncols (src/csc/ops/mul.rs:9).
    std::vector<T> operator*(const std::vector<T> &x) const {
        if (x.size() != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: `(left == right)` ncols vs x.len()");
        std::vector<T> y(nrows_);
        detail::check(detail::Abi<T>::csc_spmv(device_handle(), x.data(), x.size(), y.data(), y.size()));
        return y;
    }

    // Y = A * X for a dense ROW-MAJOR block of k vectors (x.size() == ncols * k, element (i, j) at i * k + j): one pass
    // over the matrix for all k columns, bit for bit `&A * &X` with every entry of X stored.  Panics when X has another
    // number of rows than ncols (assert_eq!, src/csc/ops/mul.rs:9).  With one or two vectors operator* is the faster call.
    std::vector<T> mul(const std::vector<T> &x, usize k) const {
        if (k == 0 || x.size() % k != 0 || x.size() / k != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.nrows (left: " + std::to_string(ncols_) +
                                                       ", right: " + std::to_string(k ? x.size() / k : 0) + ")");
        std::vector<T> y(nrows_ * k);
        detail::check(detail::Abi<T>::csc_spmm(device_handle(), k, x.data(), k, ncols_, y.data(), k, nrows_));
        return y;
    }

    // x with L x = b (the lower triangle of this matrix, `lower`) or U x = b; entries of the other triangle are ignored,
    // `unit_diagonal` takes the diagonal as ones.  Substitution on the device, bit for bit the sequential loop of
    // include/spal.h (spal_csc_trsv_*).  Panics when the matrix is not square, when b has another length than nrows,
    // and (without unit_diagonal) when a row stores no diagonal entry.
    std::vector<T> solve_triangular(const std::vector<T> &b, bool lower = true, bool unit_diagonal = false) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular: the matrix is not square (" + std::to_string(nrows_) +
                                                       " x " + std::to_string(ncols_) + ")");
        if (b.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular: b.len() = " + std::to_string(b.size()) +
                                                       " but the matrix has " + std::to_string(nrows_) + " rows");
        std::vector<T> x(nrows_);
        detail::check(detail::Abi<T>::csc_trsv(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, b.data(), b.size(),
                                               x.data(), x.size()));
        return x;
    }

    // `sweeps` Jacobi passes on the chosen triangle instead of the substitution (spal_csc_trsv_sweep_*, the sequential
    // text in include/spal.h, bit for bit): an approximate solve in launches whose rows are all independent; from
    // sweeps = levels - 1 on it IS solve_triangular's result.  Panics as solve_triangular does.
    std::vector<T> solve_triangular_sweeps(const std::vector<T> &b, bool lower, bool unit_diagonal, std::uint64_t sweeps) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular_sweeps: the matrix is not square (" +
                                                       std::to_string(nrows_) + " x " + std::to_string(ncols_) + ")");
        if (b.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_triangular_sweeps: b.len() = " + std::to_string(b.size()) +
                                                       " but the matrix has " + std::to_string(nrows_) + " rows");
        std::vector<T> x(nrows_);
        detail::check(detail::Abi<T>::csc_trsv_sweep(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, sweeps, b.data(),
                                                     b.size(), x.data(), x.size()));
        return x;
    }

    // the host-side refusals of the block solves, before any device call
    void check_block(const char *who, std::size_t len, usize k) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(who) + ": the matrix is not square (" +
                                                       std::to_string(nrows_) + " x " + std::to_string(ncols_) + ")");
        if (k == 0) throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(who) + ": k = 0 (B and X need at least one column)");
        if (len % k != 0 || len / k != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(who) + ": B.len() = " + std::to_string(len) + " is not " +
                                                       std::to_string(nrows_) + " rows of k = " + std::to_string(k));
    }

    // X with L X = B / U X = B for a ROW-MAJOR block of k right-hand sides (B.size() == nrows * k, element (i, j) at
    // i * k + j): column j of the result is bit for bit solve_triangular's result for column j of B, and all k columns
    // share one solve's launches (spal_csc_trsm_*).  Panics as solve_triangular does, and when k == 0 or B has another
    // number of rows than the matrix.
    std::vector<T> solve_triangular_block(const std::vector<T> &B, usize k, bool lower = true, bool unit_diagonal = false) const {
        check_block("solve_triangular_block", B.size(), k);
        std::vector<T> x(nrows_ * k);
        detail::check(detail::Abi<T>::csc_trsm(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, k, B.data(), k,
                                               nrows_, x.data(), k, nrows_));
        return x;
    }

    // ... and by `sweeps` Jacobi passes per column (spal_csc_trsm_sweep_*): column j is solve_triangular_sweeps' result
    // for column j of B; a pass stages the matrix once for all k columns.
    std::vector<T> solve_triangular_block_sweeps(const std::vector<T> &B, usize k, bool lower, bool unit_diagonal,
                                                 std::uint64_t sweeps) const {
        check_block("solve_triangular_block_sweeps", B.size(), k);
        std::vector<T> x(nrows_ * k);
        detail::check(detail::Abi<T>::csc_trsm_sweep(device_handle(), lower ? 0 : 1, unit_diagonal ? 1 : 0, sweeps, k,
                                                     B.data(), k, nrows_, x.data(), k, nrows_));
        return x;
    }
    // C = A * B: `impl Mul for &CscMatrix<T>` (src/csc/ops/mul.rs:5-60) on the device, bit-identical.
    CscMatrix operator*(const CscMatrix &rhs) const {
        if (ncols_ != rhs.nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "assertion failed: ncols == rhs.nrows (left: " +
                                                       std::to_string(ncols_) + ", right: " + std::to_string(rhs.nrows_) + ")");
        spal_csc_t h = nullptr;
        detail::check(spal_csc_mul(device_handle(), rhs.device_handle(), nullptr, &h));
        return adopt(h);
    }
    // C = A + B / A - B / -A: `impl Add / Sub / Neg for &CscMatrix<T>` (src/csc/ops/{add,sub,neg}.rs), bit-identical.
    CscMatrix operator+(const CscMatrix &rhs) const { return add_sub(rhs, spal_csc_add); }
    CscMatrix operator-(const CscMatrix &rhs) const { return add_sub(rhs, spal_csc_sub); }
    CscMatrix operator-() const {
        spal_csc_t h = nullptr;
        detail::check(spal_csc_neg(device_handle(), nullptr, &h));
        return adopt(h);
    }
    // The ILU(0) factor (spal_csc_ilu0): as CsrMatrix::ilu0, returned by columns.
    CscMatrix ilu0() const {
        spal_csc_t h = nullptr;
        detail::check(spal_csc_ilu0(device_handle(), nullptr, &h));
        return adopt(h);
    }
    // ILU(0) by `sweeps` row sweeps (spal_csc_ilu0_sweep): as CsrMatrix::ilu0(sweeps), returned by columns.
    CscMatrix ilu0(uint64_t sweeps) const {
        if (nrows_ != ncols_)   // before any device call
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "ilu0: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        spal_csc_t h = nullptr;
        detail::check(spal_csc_ilu0_sweep(device_handle(), sweeps, nullptr, &h));
        return adopt(h);
    }

    // The multicolour ordering (include/spal.h).  colour(): the greedy colouring of the graph of A + A^T by
    // hashed priority, exactly the sequential text, by rounds on the device.  permute(perm): B = P A P^T with
    // B[i'][j'] = A[perm[i']][perm[j']], values moved.  multicolour(): the rows numbered colour by colour, so that both
    // triangles (and those of ilu0()) have at most ncolours levels.  The results keep their permutation: ordering()
    // reads it back, to_order(v) = v[perm] and from_order() its inverse move a vector between the two numberings:
    //   auto p = a.multicolour(); auto f = p.ilu0();
    //   auto x = p.from_order(p.solve(p.to_order(b), Method::BiCgStab, &f).x);
    // Panic when the matrix is not square, perm is no permutation, or (ordering, to_order, from_order) the matrix is no
    // result of permute() / multicolour().
    Colouring colour(usize seed = 0) const {
        Colouring c{std::vector<usize>(nrows_), 0, 0};
        detail::check(spal_csc_colour(device_handle(), seed, nullptr, c.colours.data(), &c.ncolours, &c.rounds));
        return c;
    }
    CscMatrix permute(const std::vector<usize> &perm) const {
        spal_csc_t h = nullptr;
        detail::check(spal_csc_permute(device_handle(), perm.data(), perm.size(), nullptr, &h));
        return adopt(h);
    }
    CscMatrix multicolour(usize seed = 0) const {
        spal_csc_t h = nullptr;
        usize ncolours = 0;
        detail::check(spal_csc_multicolour(device_handle(), seed, nullptr, &h, &ncolours));
        return adopt(h);
    }
    Ordering ordering() const {
        Ordering o{std::vector<usize>(nrows_), 0};
        detail::check(spal_csc_ordering(device_handle(), o.perm.data(), &o.ncolours));
        return o;
    }
    std::vector<T> to_order(const std::vector<T> &v) const { return permute_vec(v, 0); }
    std::vector<T> from_order(const std::vector<T> &v) const { return permute_vec(v, 1); }
    // x with A x = b by CG (A symmetric positive definite) or BiCGStab on the device, optionally preconditioned by
    // M = ilu0() (nullptr: none), from x0 (empty: zeros); bit for bit the loops of include/spal.h (spal_csc_krylov_*).
    // Panics when the matrix is not square or a length differs; a breakdown is no panic but reason 2.
    Solution<T> solve(const std::vector<T> &b, Method method = Method::Cg, const CscMatrix *M = nullptr,
                      const std::vector<T> &x0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve: b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        Solution<T> s{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
        spal_krylov_info info;
        detail::check(detail::Abi<T>::csc_krylov(device_handle(), static_cast<int>(method), M ? M->device_handle() : nullptr,
                                                  b.data(), b.size(), s.x.data(), s.x.size(), tol, maxit, &info));
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }

    // X with A X = B for a ROW-MAJOR block of k right-hand sides (B.size() == nrows * k): k independent CG / BiCGStab
    // iterations in lockstep on shared launches (spal_csc_krylov_block_*, include/spal.h).  Column j of the result and
    // columns[j] are bit for bit solve()'s loop on column j of B, whatever k and the other columns are; a column that has
    // stopped is frozen while the others run on.  X0 empty: zeros.  Panics as solve() does, and when k == 0 or B / X0
    // are not nrows x k.
    BlockSolution<T> solve_block(const std::vector<T> &B, usize k, Method method = Method::Cg, const CscMatrix *M = nullptr,
                                 const std::vector<T> &X0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        check_block("solve_block", B.size(), k);
        if (!X0.empty() && X0.size() != B.size())
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "solve_block: X0.len() = " + std::to_string(X0.size()) +
                                                       " but B.len() = " + std::to_string(B.size()));
        BlockSolution<T> s{X0.empty() ? std::vector<T>(B.size(), T(0)) : X0, {}};
        std::vector<spal_krylov_info> info(k);
        detail::check(detail::Abi<T>::csc_krylov_block(device_handle(), static_cast<int>(method),
                                                        M ? M->device_handle() : nullptr, k, B.data(), k, nrows_,
                                                        s.x.data(), k, nrows_, tol, maxit, info.data()));
        for (const spal_krylov_info &c : info)
            s.columns.push_back(ColumnResult{c.iterations, c.reason, c.residual_sq, c.rhs_sq, c.solve_ms});
        return s;
    }

    // x with A x = b by restarted GMRES(restart) on the device, for matrices that are not symmetric; right-preconditioned
    // by M as solve() is; bit for bit the text of include/spal.h (spal_csc_gmres_*).  restart is 1 .. 256.  Reasons 0 and
    // 1 are decided on the true residual.  Panics as solve() does, and on a restart outside its range.
    Solution<T> gmres(const std::vector<T> &b, usize restart = 30, const CscMatrix *M = nullptr,
                      const std::vector<T> &x0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres: b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        if (restart == 0 || restart > 256)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres: restart = " + std::to_string(restart) + " must be 1 .. 256");
        Solution<T> s{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
        spal_krylov_info info;
        detail::check(detail::Abi<T>::csc_gmres(device_handle(), M ? M->device_handle() : nullptr, b.data(), b.size(),
                                                 s.x.data(), s.x.size(), restart, tol, maxit, &info));
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }

    // The k largest (Which::LA) or smallest (Which::SA) eigenpairs of this SYMMETRIC matrix (not checked) by thick-restart
    // Lanczos with full orthogonalisation on the device; bit for bit the text of include/spal.h (spal_csc_eigsh_*).  ncv = 0:
    // min(n, max(2k + 1, 20)); tol = 0: the element type's machine epsilon; v0 empty: the text's start vector from `seed`.
    // An eigenvalue of multiplicity > 1 is returned ONCE.  Panics on a matrix that is not square, k == 0, ncv <= k,
    // ncv > 256 or ncv > n.
    Eigenpairs<T> eigsh(usize k = 6, Which which = Which::LA, usize ncv = 0, const std::vector<T> &v0 = {}, usize seed = 0,
                        double tol = 0.0, usize maxit = 1000, bool vectors = true) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (ncv == 0) ncv = std::min<usize>(nrows_, std::max<usize>(2 * k + 1, 20));
        if (k == 0 || ncv <= k || ncv > 256 || ncv > nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh: k = " + std::to_string(k) + " and ncv = " + std::to_string(ncv) +
                                                       " must satisfy 0 < k < ncv <= min(256, " + std::to_string(nrows_) + ")");
        if (!v0.empty() && v0.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh: v0.len() = " + std::to_string(v0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        if (tol == 0.0) tol = static_cast<double>(std::numeric_limits<T>::epsilon());
        Eigenpairs<T> e{std::vector<T>(k, T(0)), std::vector<T>(k, T(0)), std::vector<T>(vectors ? nrows_ * k : 0, T(0)), 0, 0, 0, 0, 0, 0.0};
        spal_eigsh_info info;
        detail::check(detail::Abi<T>::csc_eigsh(device_handle(), k, static_cast<int>(which), ncv, v0.empty() ? nullptr : v0.data(),
                                                 v0.size(), seed, tol, maxit, e.theta.data(), k, e.resid.data(), k,
                                                 vectors ? e.x.data() : nullptr, k, nrows_, &info));
        e.pairs = info.reason == 2 ? 0 : info.reason == 3 ? info.converged : k;
        e.restarts = info.restarts;
        e.products = info.products;
        e.converged = info.converged;
        e.reason = info.reason;
        e.solve_ms = info.solve_ms;
        if (e.pairs < k) {   // pack the columns that were written
            std::vector<T> x(vectors ? nrows_ * e.pairs : 0);
            for (usize i = 0; vectors && i < nrows_; ++i)
                for (usize j = 0; j < e.pairs; ++j) x[i * e.pairs + j] = e.x[i * k + j];
            e.x.swap(x);
            e.theta.resize(e.pairs);
            e.resid.resize(e.pairs);
        }
        return e;
    }

    // eigsh on a Chebyshev polynomial of A of `degree` (1 .. 256), for CLUSTERED extreme eigenvalues (spal_csc_eigsh_filtered_*,
    // include/spal.h): automatic = true takes the interval to damp from `warmup` restarts of eigsh's own iteration, false
    // uses [lo, hi].  Convergence is decided on true residuals against tol * max(|glo|, |ghi|); tol = 0: 256 epsilons.
    FilteredEigenpairs<T> eigsh_filtered(usize k, usize degree, Which which = Which::LA, usize ncv = 0, bool automatic = true,
                                         double lo = 0.0, double hi = 0.0, usize warmup = 5, const std::vector<T> &v0 = {},
                                         usize seed = 0, double tol = 0.0, usize maxit = 1000, bool vectors = true) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (ncv == 0) ncv = std::min<usize>(nrows_, std::max<usize>(2 * k + 1, 20));
        if (k == 0 || ncv <= k || ncv > 256 || ncv > nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: k = " + std::to_string(k) + " and ncv = " + std::to_string(ncv) +
                                                       " must satisfy 0 < k < ncv <= min(256, " + std::to_string(nrows_) + ")");
        if (degree < 1 || degree > 256)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: degree = " + std::to_string(degree) + " must be 1 .. 256");
        if (!v0.empty() && v0.size() != nrows_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "eigsh_filtered: v0.len() = " + std::to_string(v0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        FilteredEigenpairs<T> f{{std::vector<T>(k, T(0)), std::vector<T>(k, T(0)), std::vector<T>(vectors ? nrows_ * k : 0, T(0)), 0, 0, 0, 0, 0, 0.0},
                                0, 0, degree, 0.0, 0.0, 0.0};
        Eigenpairs<T> &e = f.pairs;
        spal_eigsh_filter_info info;
        detail::check(detail::Abi<T>::csc_eigsh_filtered(device_handle(), k, static_cast<int>(which), ncv, v0.empty() ? nullptr : v0.data(),
                                                          v0.size(), seed, tol, maxit, degree, automatic ? 1 : 0, lo, hi, warmup,
                                                          e.theta.data(), k, e.resid.data(), k, vectors ? e.x.data() : nullptr, k,
                                                          nrows_, &info));
        e.pairs = info.reason == 2 ? 0 : info.reason == 3 ? info.converged : k;
        e.restarts = info.restarts;
        e.products = info.products;
        e.converged = info.converged;
        e.reason = info.reason;
        e.solve_ms = info.solve_ms;
        f.warm_restarts = info.warm_restarts;
        f.warm_products = info.warm_products;
        f.lo = info.lo;
        f.hi = info.hi;
        f.a0 = info.a0;
        if (e.pairs < k) {   // pack the columns that were written
            std::vector<T> x(vectors ? nrows_ * e.pairs : 0);
            for (usize i = 0; vectors && i < nrows_; ++i)
                for (usize j = 0; j < e.pairs; ++j) x[i * e.pairs + j] = e.x[i * k + j];
            e.x.swap(x);
            e.theta.resize(e.pairs);
            e.resid.resize(e.pairs);
        }
        return f;
    }

    // t_d = p(A) x: the Chebyshev polynomial of `degree` that is small on [lo, hi] and 1 at a0, outside the interval
    // (spal_csc_cheb_apply_*): the text of include/spal.h bit for bit.  Panics as the library refuses.
    std::vector<T> cheb_apply(const std::vector<T> &x, usize degree, double lo, double hi, double a0) const {
        std::vector<T> out(nrows_, T(0));
        detail::check(detail::Abi<T>::csc_cheb_apply(device_handle(), x.data(), x.size(), out.data(), out.size(), degree, lo, hi, a0));
        return out;
    }

    // (glo, ghi): Gershgorin's enclosure of the spectrum, in double (spal_csc_gershgorin)
    std::pair<double, double> gershgorin() const {
        double lo = 0.0, hi = 0.0;
        detail::check(spal_csc_gershgorin(device_handle(), &lo, &hi));
        return {lo, hi};
    }

    // The KPM moments mu[i * k + j] = z_j^T T_i(B) z_j, i = 0 .. degree, of k probe columns (spal_csc_kpm_moments_*,
    // include/spal.h): the text bit for bit, in double.  z empty: hashed +-1 probes from `seed`, else a ROW-MAJOR
    // nrows x k block.  automatic: Gershgorin's bounds with a margin, else [lo, hi], which must enclose the spectrum.
    // The matrix must be symmetric (not checked).  Panics as the library refuses.
    KpmMoments kpm_moments(usize degree, usize k = 8, usize seed = 0, bool automatic = true, double lo = 0.0, double hi = 0.0,
                           const std::vector<T> &z = {}) const {
        KpmMoments out;
        out.mu.assign((degree + 1) * k, 0.0);
        detail::check(detail::Abi<T>::csc_kpm_moments(device_handle(), degree, k, seed, automatic ? 1 : 0, lo, hi,
                                                      z.empty() ? nullptr : z.data(), k ? z.size() / k : 0, k, out.mu.data(),
                                                      out.mu.size(), &out.info));
        return out;
    }
    // ... with the probes in device memory (z_dev == nullptr: hashed), enqueued on `stream`; synchronises once, at its end
    KpmMoments kpm_moments_dev(usize degree, usize k, usize seed, bool automatic, double lo, double hi, const T *z_dev, usize ldz,
                               void *stream) const {
        KpmMoments out;
        out.mu.assign((degree + 1) * k, 0.0);
        detail::check(detail::Abi<T>::csc_kpm_moments_dev(device_handle(), degree, k, seed, automatic ? 1 : 0, lo, hi, z_dev, ldz,
                                                          out.mu.data(), out.mu.size(), stream, &out.info));
        return out;
    }

    // X with A X = B for a ROW-MAJOR block of k right-hand sides by restarted GMRES(restart): k independent iterations in
    // lockstep on shared launches, with cycles common to the block (spal_csc_gmres_block_*, include/spal.h).  Column j
    // of the result and columns[j] are bit for bit gmres()'s text on column j of B, whatever k and the other columns are.
    // X0 empty: zeros.  Panics as gmres() does, and when k == 0 or B / X0 are not nrows x k.
    BlockSolution<T> gmres_block(const std::vector<T> &B, usize k, usize restart = 30, const CscMatrix *M = nullptr,
                                 const std::vector<T> &X0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        check_block("gmres_block", B.size(), k);
        if (!X0.empty() && X0.size() != B.size())
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres_block: X0.len() = " + std::to_string(X0.size()) +
                                                       " but B.len() = " + std::to_string(B.size()));
        if (restart == 0 || restart > 256)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "gmres_block: restart = " + std::to_string(restart) + " must be 1 .. 256");
        BlockSolution<T> s{X0.empty() ? std::vector<T>(B.size(), T(0)) : X0, {}};
        std::vector<spal_krylov_info> info(k);
        detail::check(detail::Abi<T>::csc_gmres_block(device_handle(), M ? M->device_handle() : nullptr, k, B.data(), k,
                                                       nrows_, s.x.data(), k, nrows_, restart, tol, maxit, info.data()));
        for (const spal_krylov_info &c : info)
            s.columns.push_back(ColumnResult{c.iterations, c.reason, c.residual_sq, c.rhs_sq, c.solve_ms});
        return s;
    }

    // x with (A - shift I) x = b by MINRES on the device, for a SYMMETRIC matrix that may be indefinite (not checked); M,
    // when given, symmetric positive definite and applied as solve() applies it; bit for bit the text of include/spal.h
    // (spal_csc_minres_*).  The residual estimate never grows, so reason 1 still returns the best iterate.  Panics as
    // solve() does, and on a shift that is not finite.
    Solution<T> minres(const std::vector<T> &b, const CscMatrix *M = nullptr, double shift = 0.0, const std::vector<T> &x0 = {},
                       double tol = 1e-8, usize maxit = 1000) const {
        if (nrows_ != ncols_)
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres: the matrix is not square (" + std::to_string(nrows_) + " x " +
                                                       std::to_string(ncols_) + ")");
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres: b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the matrix has " +
                                                       std::to_string(nrows_) + " rows");
        if (!(shift - shift == 0.0)) throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres: shift must be finite");
        Solution<T> s{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
        spal_krylov_info info;
        detail::check(detail::Abi<T>::csc_minres(device_handle(), M ? M->device_handle() : nullptr, shift, b.data(),
                                                  b.size(), s.x.data(), s.x.size(), tol, maxit, &info));
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }

    // X with (A - shift I) X = B for a ROW-MAJOR block of k right-hand sides by MINRES: k independent iterations in
    // lockstep on shared launches (spal_csc_minres_block_*, include/spal.h).  Column j of the result and columns[j] are
    // bit for bit minres()'s text on column j of B, whatever k and the other columns are.  X0 empty: zeros.  Panics as
    // minres() does, and when k == 0 or B / X0 are not nrows x k.
    BlockSolution<T> minres_block(const std::vector<T> &B, usize k, const CscMatrix *M = nullptr, double shift = 0.0,
                                  const std::vector<T> &X0 = {}, double tol = 1e-8, usize maxit = 1000) const {
        check_block("minres_block", B.size(), k);
        if (!X0.empty() && X0.size() != B.size())
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres_block: X0.len() = " + std::to_string(X0.size()) +
                                                       " but B.len() = " + std::to_string(B.size()));
        if (!(shift - shift == 0.0)) throw Panic(SPAL_ERR_INVALID_ARGUMENT, "minres_block: shift must be finite");
        BlockSolution<T> s{X0.empty() ? std::vector<T>(B.size(), T(0)) : X0, {}};
        std::vector<spal_krylov_info> info(k);
        detail::check(detail::Abi<T>::csc_minres_block(device_handle(), M ? M->device_handle() : nullptr, shift, k, B.data(),
                                                        k, nrows_, s.x.data(), k, nrows_, tol, maxit, info.data()));
        for (const spal_krylov_info &c : info)
            s.columns.push_back(ColumnResult{c.iterations, c.reason, c.residual_sq, c.rhs_sq, c.solve_ms});
        return s;
    }
    // CscMatrix::from(&csr)  (src/csc/conv/csr.rs:4-52) and CscMatrix::from(&coo)
    // (src/csc/conv/coo.rs:3-116), both on the device.
    static CscMatrix from(const CsrMatrix<T> &csr, int device = 0) {
        spal_csc_t h = nullptr;
        detail::check(spal_csr_to_csc(csr.device_handle(device), &h));
        return adopt(h);
    }
    static CscMatrix from(const CooMatrix<T> &coo, int device = 0);

  private:
    friend class CsrMatrix<T>;
    struct Trusted {};
    CscMatrix(Trusted, usize nrows, usize ncols, std::vector<usize> cp, std::vector<usize> ri,
              std::vector<T> va)
        : nrows_(nrows), ncols_(ncols), colptr_(std::move(cp)), rowind_(std::move(ri)),
          values_(std::move(va)) {}
    CscMatrix add_sub(const CscMatrix &rhs, int (*op)(spal_csc_t, spal_csc_t, void *, spal_csc_t *)) const {
        detail::check_same_shape(nrows_, ncols_, rhs.nrows_, rhs.ncols_);
        spal_csc_t h = nullptr;
        detail::check(op(device_handle(), rhs.device_handle(), nullptr, &h));
        return adopt(h);
    }
    std::vector<T> permute_vec(const std::vector<T> &v, int direction) const {
        std::vector<T> y(v.size());
        detail::check(detail::Abi<T>::csc_permute_vec(device_handle(), v.data(), v.size(), y.data(), y.size(), direction));
        return y;
    }
    static CscMatrix adopt(spal_csc_t h) {
        std::unique_ptr<spal_csc, detail::CscDeleter> guard(h);
        uint64_t nr = 0, nc = 0, nz = 0;
        int es = 0;
        detail::check(spal_csc_shape(h, &nr, &nc, &nz, &es));
        std::vector<usize> cp(nc + 1), ri(nz);
        std::vector<T> va(nz);
        detail::check(detail::Abi<T>::csc_download(h, cp.data(), ri.data(), va.data()));
        CscMatrix out(Trusted{}, nr, nc, std::move(cp), std::move(ri), std::move(va));
        out.dev_ = std::move(guard);
        return out;
    }
    usize nrows_, ncols_;
    std::vector<usize> colptr_, rowind_;
    std::vector<T> values_;
    mutable std::unique_ptr<spal_csc, detail::CscDeleter> dev_;
};

// ---------------------------------------------------------------------------
// CooMatrix<T>                                      reference src/coo.rs:53-57
// Insertion order is significant: the conversion sums duplicates in it.
// ---------------------------------------------------------------------------
template <typename T>
class CooMatrix {
  public:
    // CooMatrix::new                                         src/coo.rs:104-112
    CooMatrix(usize nrows, usize ncols) : nrows_(nrows), ncols_(ncols) {
        if (!(nrows > 0)) throw Panic(SPAL_ERR_INVARIANT, "assertion failed: nrows > 0");
        if (!(ncols > 0)) throw Panic(SPAL_ERR_INVARIANT, "assertion failed: ncols > 0");
    }
    static CooMatrix with_capacity(usize nrows, usize ncols, usize capacity) {
        CooMatrix m(nrows, ncols);
        m.rows_.reserve(capacity); m.cols_.reserve(capacity); m.vals_.reserve(capacity);
        return m;
    }
    // CooMatrix::with_triplets                               src/coo.rs:260-288
    static CooMatrix with_triplets(usize nrows, usize ncols, const std::vector<usize> &rowind,
                                   const std::vector<usize> &colind, const std::vector<T> &values) {
        CooMatrix m(nrows, ncols);
        if (rowind.size() != values.size()) throw Panic(SPAL_ERR_INVARIANT, "assertion failed: rowind.len() == values.len()");
        if (colind.size() != values.size()) throw Panic(SPAL_ERR_INVARIANT, "assertion failed: colind.len() == values.len()");
        for (usize r : rowind) if (!(r < nrows)) throw Panic(SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: *row < nrows");
        for (usize c : colind) if (!(c < ncols)) throw Panic(SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: *col < ncols");
        m.rows_ = rowind; m.cols_ = colind; m.vals_ = values;
        return m;
    }
    // CooMatrix::with_entries                                src/coo.rs:204-221
    static CooMatrix with_entries(usize nrows, usize ncols, const std::vector<std::tuple<usize, usize, T>> &entries) {
        CooMatrix m(nrows, ncols);
        for (const auto &e : entries) m.push(std::get<0>(e), std::get<1>(e), std::get<2>(e));
        return m;
    }
    // CooMatrix::push                                        src/coo.rs:431-435
    void push(usize row, usize col, T value) {
        if (!(row < nrows_)) throw Panic(SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: row < self.nrows");
        if (!(col < ncols_)) throw Panic(SPAL_ERR_INDEX_OUT_OF_BOUNDS, "assertion failed: col < self.ncols");
        rows_.push_back(row); cols_.push_back(col); vals_.push_back(value);
    }
    usize nrows() const { return nrows_; }
    usize ncols() const { return ncols_; }
    usize length() const { return vals_.size(); }
    // the three components of `iter()` (src/coo.rs:491-495), unzipped
    const std::vector<usize> &rows() const { return rows_; }
    const std::vector<usize> &cols() const { return cols_; }
    const std::vector<T> &vals() const { return vals_; }

  private:
    usize nrows_, ncols_;
    std::vector<usize> rows_, cols_;
    std::vector<T> vals_;
};

template <typename T>
CsrMatrix<T> CsrMatrix<T>::from(const CooMatrix<T> &coo, int device) {
    spal_csr_t h = nullptr;
    detail::check(detail::Abi<T>::coo_to_csr(device, coo.nrows(), coo.ncols(), coo.length(),
                                             coo.rows().data(), coo.cols().data(), coo.vals().data(), &h));
    return adopt(h);
}

template <typename T>
CsrMatrix<T> CsrMatrix<T>::from(const CscMatrix<T> &csc, int device) {
    spal_csr_t h = nullptr;
    detail::check(spal_csc_to_csr(csc.device_handle(device), &h));
    return adopt(h);
}

template <typename T>
CscMatrix<T> CscMatrix<T>::from(const CooMatrix<T> &coo, int device) {
    spal_csc_t h = nullptr;
    detail::check(detail::Abi<T>::coo_to_csc(device, coo.nrows(), coo.ncols(), coo.length(),
                                             coo.rows().data(), coo.cols().data(), coo.vals().data(), &h));
    return adopt(h);
}

// ---------------------------------------------------------------------------
// Fsai<T>: G ~ L^-1 on a prescribed pattern, M^-1 = Gt G    not in the reference (include/spal.h, spal_fsai_*)
// ---------------------------------------------------------------------------
namespace detail {
struct FsaiDeleter { void operator()(spal_fsai *h) const { spal_fsai_destroy(h); } };
inline int fsai_apply(spal_fsai_t f, const double *b, usize n, double *x) { return spal_fsai_apply_f64(f, b, n, x, n); }
inline int fsai_apply(spal_fsai_t f, const float *b, usize n, float *x) { return spal_fsai_apply_f32(f, b, n, x, n); }
inline int fsai_row(usize m, const double *b, double *g, int *rej) { return spal_fsai_row_f64(m, b, g, rej); }
inline int fsai_row(usize m, const float *b, float *g, int *rej) { return spal_fsai_row_f32(m, b, g, rej); }
#define SPALINALG_FSAI_SOLVERS(kind, T, sfx)                                                                            \
    inline int krylov_fsai(spal_##kind##_t a, int method, spal_fsai_t f, const T *b, usize n, T *x, double tol,         \
                           usize maxit, spal_krylov_info *info) {                                                       \
        return spal_##kind##_krylov_fsai_##sfx(a, method, f, b, n, x, n, tol, maxit, info);                             \
    }                                                                                                                   \
    inline int minres_fsai(spal_##kind##_t a, spal_fsai_t f, double shift, const T *b, usize n, T *x, double tol,       \
                           usize maxit, spal_krylov_info *info) {                                                       \
        return spal_##kind##_minres_fsai_##sfx(a, f, shift, b, n, x, n, tol, maxit, info);                              \
    }
SPALINALG_FSAI_SOLVERS(csr, double, f64)
SPALINALG_FSAI_SOLVERS(csr, float, f32)
SPALINALG_FSAI_SOLVERS(csc, double, f64)
SPALINALG_FSAI_SOLVERS(csc, float, f32)
#undef SPALINALG_FSAI_SOLVERS
}  // namespace detail

// (g, rejected): the text's Cholesky and back-substitution on ONE local system, on the host (spal_fsai_row_*); b_lower
// is the lower triangle packed by rows, m (m + 1) / 2 values.
template <typename T>
std::pair<std::vector<T>, bool> fsai_row(usize m, const std::vector<T> &b_lower) {
    if (b_lower.size() != m * (m + 1) / 2)
        throw Panic(SPAL_ERR_INVALID_ARGUMENT, "fsai_row: b_lower.len() = " + std::to_string(b_lower.size()) + " is not m (m + 1) / 2");
    std::vector<T> g(m);
    int rejected = 0;
    detail::check(detail::fsai_row(m, b_lower.data(), g.data(), &rejected));
    return {std::move(g), rejected != 0};
}

// The FSAI factor of a square, symmetric positive definite matrix on the lower triangle of `pattern`'s structure
// (nullptr: the matrix's own), built on the device and owned by this object; it outlives the matrix.  The matrix's
// option "fsai_max_row" (1 .. 64, default 32) caps a row's local system.  apply(v) = Gt (G v), two SpMVs; solve() and
// minres() are a.solve() / a.minres() with this factor as M, bit for bit the texts of include/spal.h.
template <typename T>
class Fsai {
  public:
    explicit Fsai(const CsrMatrix<T> &a, const CsrMatrix<T> *pattern = nullptr, int device = 0) : nrows_(a.nrows()) {
        spal_fsai_t h = nullptr;
        detail::check(spal_csr_fsai_setup(a.device_handle(device), pattern ? pattern->device_handle(device) : nullptr, nullptr, &h));
        h_.reset(h);
    }
    explicit Fsai(const CscMatrix<T> &a, const CscMatrix<T> *pattern = nullptr, int device = 0) : nrows_(a.nrows()) {
        spal_fsai_t h = nullptr;
        detail::check(spal_csc_fsai_setup(a.device_handle(device), pattern ? pattern->device_handle(device) : nullptr, nullptr, &h));
        h_.reset(h);
    }
    spal_fsai_t handle() const { return h_.get(); }
    usize nrows() const { return nrows_; }
    std::string describe() const {
        std::string buf(4096, '\0');
        detail::check(spal_fsai_describe(h_.get(), &buf[0], buf.size()));
        buf.resize(buf.find('\0'));
        return buf;
    }
    std::vector<T> apply(const std::vector<T> &b) const {
        std::vector<T> x(b.size());
        detail::check(detail::fsai_apply(h_.get(), b.data(), b.size(), x.data()));
        return x;
    }
    template <typename Matrix>
    Solution<T> solve(const Matrix &a, const std::vector<T> &b, Method method = Method::Cg, const std::vector<T> &x0 = {},
                      double tol = 1e-8, usize maxit = 1000) const {
        Solution<T> s = start("solve", b, x0);
        spal_krylov_info info;
        detail::check(detail::krylov_fsai(a.device_handle(), (int)method, h_.get(), b.data(), b.size(), s.x.data(), tol, maxit, &info));
        return finish(std::move(s), info);
    }
    template <typename Matrix>
    Solution<T> minres(const Matrix &a, const std::vector<T> &b, double shift = 0.0, const std::vector<T> &x0 = {},
                       double tol = 1e-8, usize maxit = 1000) const {
        Solution<T> s = start("minres", b, x0);
        spal_krylov_info info;
        detail::check(detail::minres_fsai(a.device_handle(), h_.get(), shift, b.data(), b.size(), s.x.data(), tol, maxit, &info));
        return finish(std::move(s), info);
    }

  private:
    Solution<T> start(const char *what, const std::vector<T> &b, const std::vector<T> &x0) const {
        if (b.size() != nrows_ || (!x0.empty() && x0.size() != nrows_))
            throw Panic(SPAL_ERR_INVALID_ARGUMENT, std::string(what) + ": b.len() = " + std::to_string(b.size()) + " and x0.len() = " +
                                                       std::to_string(x0.size()) + " but the factor has " + std::to_string(nrows_) + " rows");
        return Solution<T>{x0.empty() ? std::vector<T>(nrows_, T(0)) : x0, 0, 0, 0.0, 0.0, 0.0};
    }
    static Solution<T> finish(Solution<T> s, const spal_krylov_info &info) {
        s.iterations = info.iterations;
        s.reason = info.reason;
        s.residual_sq = info.residual_sq;
        s.rhs_sq = info.rhs_sq;
        s.solve_ms = info.solve_ms;
        return s;
    }
    usize nrows_;
    std::unique_ptr<spal_fsai, detail::FsaiDeleter> h_;
};

}  // namespace spalinalg

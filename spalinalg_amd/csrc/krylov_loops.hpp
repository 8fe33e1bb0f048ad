// krylov_loops.hpp -- the CG, the BiCGStab and the MINRES loop of include/spal.h as the sequence of launches a driver
// enqueues, written ONCE for spal_krylov.hip (one right-hand side) and spal_krylov_block.hip (a block of them): DESIGN
// 3.14, 3.27.  There is no
// HIP in here -- the names of the fused updates (VecOp) and of the scalar steps (FinOp), three function templates over a
// driver type R, nothing else -- so tests/cpp/test_krylov_loops.cpp compiles it with a plain C++ compiler and compares
// what a recording R was asked to enqueue with the sequences written out in its text.  (Not installed.)
//
// R provides, all resolved statically (every call below returns 0, or a status that ends the call at once):
//   null()                   the operand an update does not name (nullptr; {nullptr, 0})
//   B(), X(), work(i)        the call's right-hand side and solution, work vector i
//   mul(in, out)             out = A in
//   prec(in, out)            out = M^-1 in (out != in); only called when preconditioned()
//   v<OP>(a, b, c, d, x, y)  update OP, fused with the first level of the dots that follow it
//   v<OP>(a, .., x, y, z)    the same with a third written operand (V_MR_WX alone; only the MINRES loop asks for it)
//   f<OP>(unpreconditioned)  the upper levels of those dots and the scalar step OP
//   copy(dst, src), zero(dst)
//   poll()                   the scalars to the host: the one place a call waits for the device
//   all_stopped()            what the last poll found (false before the first)
//   polls()                  how many there were
// Work vectors by number: r, q, p, then z (CG) or rhat, v, t, ph, sh (BiCGStab); z, ph and sh are vectors of their own
// only with a preconditioner.  MINRES: v, the ring r1 / r2 / t (three buffers), the ring w1 / w2 (two: w is written over
// w1, which the text never reads again), then y with a preconditioner.
#pragma once

#include <cstdint>

namespace spal {

// ---- the first level, fused with the vector update in front of it ---------------------------------------------------
enum VecOp {
    V_DOT,      // d0 = a . b
    V_DOT2,     // d0 = a . b, d1 = a . a
    V_INIT,     // y = a - b;  d0 = y . y, d1 = a . a                                   (r = b - q;  rr, bb)
    V_COPY_DOT, // y = b;  d0 = a . b                                                   (p = z;  rz)
    V_CG_XR,    // x += alpha * a;  y -= alpha * b;  d0 = y . y                         (x, r;  rr)
    V_CG_P,     // y = a + beta * y                                                     (p = z + beta p)
    V_BI_P,     // y = a + beta * (y - omega * b)                                       (p = r + beta (p - omega v))
    V_BI_S,     // y = a - alpha * b;  d0 = y . y                                       (s = r - alpha v;  ss)
    V_BI_HALF,  // only when `half`:  x += alpha * a;  y = b                            (x += alpha ph;  r = s)
    V_BI_XR,    // x = (x + alpha * a) + omega * b;  y = c - omega * d;  d0 = y . y      (x, r;  rr)
    // MINRES (sg = T(shift); c1, c2, oldeps, delta, denom, phi, s: the call's scalars)
    V_MR_R0,    // y = a - (b - sg * c);  d0 = y . y, d1 = a . a                        (r2 = b - (q - sg x))
    V_MR_V,     // y = a * s                                                            (v = y s)
    V_MR_T1,    // y = (y - sg * a) - c1 * b;  d0 = a . y                               (t = (q - sg v) - c1 r1;  alfa)
    V_MR_T2,    // y = y - c2 * a;  d0 = y . y                                          (t -= c2 r2;  beta^2 when y is r2)
    V_MR_T2_PRE,// y = y - c2 * a                                                       (the same in front of M^-1)
    V_MR_WX,    // y = ((z - oldeps * y) - delta * b) * denom;  x += phi * y;  not stopped: z = a * s   (w, x, next v)
};

// ---- the scalar step that follows a dot: thread 0 of the launch that walked the upper levels --------------------------
enum FinOp { F_STORE, F_INIT, F_RZ, F_ALPHA_CG, F_TEST_CG, F_BETA, F_RHO, F_ALPHA_BI, F_HALF, F_OMEGA, F_TEST_BI,
             F_MR_BB,     // bb = d0                                              (preconditioned: bb = dot(b, M^-1 b))
             F_MR_INIT,   // bb (= d1 when unpreconditioned), thr, it = 0, beta = sqrt(d0), phibar, pp, test, s; the state
             F_MR_ALFA,   // alfa = d0;  c2 = alfa / beta                          (and `half` is cleared)
             F_MR_ROT };  // oldb, beta = sqrt(d0), it, the rotation, phi, phibar, denom, pp, test; s, c1 or `half`

#define KRYLOV_TRY(expr)               \
    do {                               \
        const int st_ = (expr);        \
        if (st_ != 0) return st_;      \
    } while (0)

// r = b - A x;  rr, bb;  it = 0;  test
template <typename R>
int krylov_start(R &run) {
    const auto none = run.null();
    KRYLOV_TRY(run.mul(run.X(), run.work(1)));
    KRYLOV_TRY((run.template v<V_INIT>(run.B(), run.work(1), none, none, none, run.work(0))));
    return run.template f<F_INIT>(0);
}

// The outer rule of both loops: min(check_every, maxit - enqueued) iterations, then a poll, until every column has
// stopped or maxit iterations are enqueued; one poll at least (maxit = 0: the test after r0 has decided).
template <typename R, typename Iteration>
int krylov_batches(R &run, uint64_t maxit, uint64_t check_every, Iteration iteration) {
    uint64_t enqueued = 0;
    while (enqueued < maxit && !run.all_stopped()) {
        const uint64_t batch = check_every < maxit - enqueued ? check_every : maxit - enqueued;
        for (uint64_t i = 0; i < batch; ++i) KRYLOV_TRY(iteration());
        enqueued += batch;
        KRYLOV_TRY(run.poll());
    }
    if (!run.polls()) KRYLOV_TRY(run.poll());
    return 0;
}

template <typename R>
int cg_loop(R &run, uint64_t maxit, uint64_t check_every) {
    const bool pre = run.preconditioned();
    const auto none = run.null();
    const auto x = run.X(), r = run.work(0), q = run.work(1), p = run.work(2), z = pre ? run.work(3) : r;
    if (pre) KRYLOV_TRY(run.prec(r, z));
    KRYLOV_TRY((run.template v<V_COPY_DOT>(r, z, none, none, none, p)));   // p = z;  rz
    KRYLOV_TRY((run.template f<F_RZ>(0)));
    return krylov_batches(run, maxit, check_every, [&]() -> int {
        KRYLOV_TRY(run.mul(p, q));
        KRYLOV_TRY((run.template v<V_DOT>(p, q, none, none, none, none)));
        KRYLOV_TRY((run.template f<F_ALPHA_CG>(0)));
        KRYLOV_TRY((run.template v<V_CG_XR>(p, q, none, none, x, r)));      // x, r;  rr
        KRYLOV_TRY((run.template f<F_TEST_CG>(pre ? 0 : 1)));              // it, test (and beta when z is r)
        if (pre) {
            KRYLOV_TRY(run.prec(r, z));
            KRYLOV_TRY((run.template v<V_DOT>(r, z, none, none, none, none)));
            KRYLOV_TRY((run.template f<F_BETA>(0)));
        }
        return run.template v<V_CG_P>(z, none, none, none, none, p);
    });
}

template <typename R>
int bicgstab_loop(R &run, uint64_t maxit, uint64_t check_every) {
    const bool pre = run.preconditioned();
    const auto none = run.null();
    const auto x = run.X(), r = run.work(0), p = run.work(2), rhat = run.work(3), vv = run.work(4), t = run.work(5);
    const auto sv = run.work(1);   // q is free once r exists
    const auto ph = pre ? run.work(6) : p, sh = pre ? run.work(7) : sv;
    KRYLOV_TRY(run.copy(rhat, r));
    KRYLOV_TRY(run.zero(vv));
    KRYLOV_TRY(run.zero(p));
    return krylov_batches(run, maxit, check_every, [&]() -> int {
        KRYLOV_TRY((run.template v<V_DOT>(rhat, r, none, none, none, none)));
        KRYLOV_TRY((run.template f<F_RHO>(0)));
        KRYLOV_TRY((run.template v<V_BI_P>(r, vv, none, none, none, p)));
        if (pre) KRYLOV_TRY(run.prec(p, ph));
        KRYLOV_TRY(run.mul(ph, vv));
        KRYLOV_TRY((run.template v<V_DOT>(rhat, vv, none, none, none, none)));
        KRYLOV_TRY((run.template f<F_ALPHA_BI>(0)));
        KRYLOV_TRY((run.template v<V_BI_S>(r, vv, none, none, none, sv)));   // s;  ss
        KRYLOV_TRY((run.template f<F_HALF>(0)));                            // it;  the half-step exit
        KRYLOV_TRY((run.template v<V_BI_HALF>(ph, sv, none, none, x, r)));   // ... applied, where taken
        if (pre) KRYLOV_TRY(run.prec(sv, sh));
        KRYLOV_TRY(run.mul(sh, t));
        KRYLOV_TRY((run.template v<V_DOT2>(t, sv, none, none, none, none)));   // t . s, t . t
        KRYLOV_TRY((run.template f<F_OMEGA>(0)));
        KRYLOV_TRY((run.template v<V_BI_XR>(ph, sh, sv, t, x, r)));          // x, r;  rr
        return run.template f<F_TEST_BI>(0);
    });
}

// ---- MINRES on (A - shift I) x = b -----------------------------------------------------------------------
// bb, r2 = b - (A - sg I) x, y = M^-1 r2, beta, pp, it = 0, test;  r1 = w = w2 = 0;  v = y / beta
template <typename R>
int minres_start(R &run) {
    const bool pre = run.preconditioned();
    const auto none = run.null();
    const auto v = run.work(0), r1 = run.work(1), r2 = run.work(2);
    const auto y = pre ? run.work(6) : r2;
    if (pre) {
        KRYLOV_TRY(run.prec(run.B(), y));
        KRYLOV_TRY((run.template v<V_DOT>(run.B(), y, none, none, none, none)));
        KRYLOV_TRY((run.template f<F_MR_BB>(0)));
    }
    KRYLOV_TRY(run.mul(run.X(), r2));
    KRYLOV_TRY((run.template v<V_MR_R0>(run.B(), r2, run.X(), none, none, r2)));   // in place: q becomes r2
    if (pre) {
        KRYLOV_TRY(run.prec(r2, y));
        KRYLOV_TRY((run.template v<V_DOT>(r2, y, none, none, none, none)));
    }
    KRYLOV_TRY((run.template f<F_MR_INIT>(pre ? 0 : 1)));
    KRYLOV_TRY(run.zero(r1));
    KRYLOV_TRY(run.zero(run.work(4)));
    KRYLOV_TRY(run.zero(run.work(5)));
    return run.template v<V_MR_V>(y, none, none, none, none, v);
}

// Iteration j: r1, r2, t are ring buffers j, j + 1, j + 2 (mod 3) of work(1 .. 3) -- the product writes the next t into
// the buffer r1 has just left -- and w1, w2 are j, j + 1 (mod 2) of work(4 .. 5).  Nothing is copied.
template <typename R>
int minres_loop(R &run, uint64_t maxit, uint64_t check_every) {
    const bool pre = run.preconditioned();
    const auto none = run.null();
    const auto x = run.X(), v = run.work(0);
    uint64_t j = 0;
    return krylov_batches(run, maxit, check_every, [&]() -> int {
        const auto r1 = run.work(1 + (int)(j % 3)), r2 = run.work(1 + (int)((j + 1) % 3)), t = run.work(1 + (int)((j + 2) % 3));
        const auto w1 = run.work(4 + (int)(j % 2)), w2 = run.work(4 + (int)((j + 1) % 2));
        const auto y = pre ? run.work(6) : t;
        ++j;
        KRYLOV_TRY(run.mul(v, t));
        KRYLOV_TRY((run.template v<V_MR_T1>(v, r1, none, none, none, t)));     // the shift, c1 r1;  alfa
        KRYLOV_TRY((run.template f<F_MR_ALFA>(0)));
        if (pre) {
            KRYLOV_TRY((run.template v<V_MR_T2_PRE>(r2, none, none, none, none, t)));
            KRYLOV_TRY(run.prec(t, y));
            KRYLOV_TRY((run.template v<V_DOT>(t, y, none, none, none, none)));
        } else {
            KRYLOV_TRY((run.template v<V_MR_T2>(r2, none, none, none, none, t)));   // t is the new r2;  beta^2
        }
        KRYLOV_TRY((run.template f<F_MR_ROT>(0)));                              // it, the rotation, the test
        return run.template v<V_MR_WX>(y, w2, none, none, x, w1, v);            // w over w1, x, the next v in place
    });
}

#undef KRYLOV_TRY

}  // namespace spal

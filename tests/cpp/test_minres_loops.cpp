// minres_start and minres_loop of spalinalg_amd/csrc/krylov_loops.hpp, driven by a recording driver: no HIP, no device.
// Every mul / prec / v<OP> / f<OP> / zero / poll appends its name and its operands' names to a string, and all_stopped()
// follows a script.  Prints one line per scenario, "name: status | trace"; tests/test_minres_loops.py compares the lines
// with the sequences written out there.
#include "krylov_loops.hpp"

#include <cstdio>
#include <string>

using namespace spal;

namespace {

const char *const kVecNames[] = {"V_DOT", "V_DOT2", "V_INIT", "V_COPY_DOT", "V_CG_XR", "V_CG_P", "V_BI_P", "V_BI_S", "V_BI_HALF",
                                 "V_BI_XR", "V_MR_R0", "V_MR_V", "V_MR_T1", "V_MR_T2", "V_MR_T2_PRE", "V_MR_WX"};
const char *const kFinNames[] = {"F_STORE", "F_INIT", "F_RZ", "F_ALPHA_CG", "F_TEST_CG", "F_BETA", "F_RHO", "F_ALPHA_BI", "F_HALF",
                                 "F_OMEGA", "F_TEST_BI", "F_MR_BB", "F_MR_INIT", "F_MR_ALFA", "F_MR_ROT"};
const char *const kWork[] = {"v", "ra", "rb", "rc", "wa", "wb", "y"};   // the two rings by buffer, not by role

struct Recorder {
    bool pre = false;
    uint64_t stop_at_poll = 0;   // all_stopped() from this poll on; 0: never
    uint64_t fail_at = 0;        // the call with this number (from 1) returns 7 and is not recorded; 0: none
    uint64_t calls = 0, npolls = 0;
    std::string trace;

    int say(const std::string &what) {
        if (++calls == fail_at) return 7;
        if (!trace.empty()) trace += ' ';
        trace += what;
        return 0;
    }
    static const char *null() { return "-"; }
    const char *B() const { return "B"; }
    const char *X() const { return "X"; }
    const char *work(int i) const { return (i < 0 || i > 6 || (!pre && i == 6)) ? "NO-SUCH-VECTOR" : kWork[i]; }
    bool preconditioned() const { return pre; }
    int mul(const char *in, const char *out) { return say(std::string("mul(") + in + "," + out + ")"); }
    int prec(const char *in, const char *out) { return say(std::string("prec(") + in + "," + out + ")"); }
    template <int OP>
    int v(const char *a, const char *b, const char *c, const char *d, const char *x, const char *y, const char *z = nullptr) {
        return say(std::string(kVecNames[OP]) + "(" + a + "," + b + "," + c + "," + d + "," + x + "," + y + (z ? std::string(",") + z : "") + ")");
    }
    template <int OP>
    int f(int unpreconditioned = 0) {
        return say(std::string(kFinNames[OP]) + "(" + std::to_string(unpreconditioned) + ")");
    }
    int zero(const char *dst) { return say(std::string("zero(") + dst + ")"); }
    int poll() {
        ++npolls;
        return say("poll");
    }
    bool all_stopped() const { return stop_at_poll && npolls >= stop_at_poll; }
    uint64_t polls() const { return npolls; }
};

void loop(const char *name, bool pre, uint64_t maxit, uint64_t check_every, uint64_t stop_at_poll = 0, uint64_t fail_at = 0) {
    Recorder r;
    r.pre = pre;
    r.stop_at_poll = stop_at_poll;
    r.fail_at = fail_at;
    const int status = minres_loop(r, maxit, check_every);
    printf("%s: %d | %s\n", name, status, r.trace.c_str());
}

}  // namespace

int main() {
    static_assert(sizeof kVecNames / sizeof *kVecNames == V_MR_WX + 1 && sizeof kFinNames / sizeof *kFinNames == F_MR_ROT + 1,
                  "the new names stand at the END of VecOp and FinOp");
    static_assert(V_BI_XR == 9 && F_TEST_BI == 10, "the names of CG and BiCGStab keep their values");
    for (int pre = 0; pre < 2; ++pre) {
        Recorder r;
        r.pre = pre;
        const int status = minres_start(r);
        printf("start_%s: %d | %s\n", pre ? "pre" : "plain", status, r.trace.c_str());
    }
    loop("plain", false, 7, 7);
    loop("pre", true, 7, 7);
    loop("0_8", false, 0, 8);
    loop("5_2", false, 5, 2);
    loop("5_8", false, 5, 8);
    loop("40_1_stop3", false, 40, 1, 3);
    loop("fail4", false, 5, 2, 0, 4);
    return 0;
}

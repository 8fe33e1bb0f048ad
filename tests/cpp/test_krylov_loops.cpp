// The CG and BiCGStab loops of spalinalg_amd/csrc/krylov_loops.hpp, driven by a recording driver: no HIP, no device.
// Every mul / prec / v<OP> / f<OP> / copy / zero / poll appends its name and its operands' names to a string, and
// all_stopped() follows a script.  Prints one line per scenario, "name: status | trace"; tests/test_krylov_loops.py
// compares the lines with the sequences written out there.
#include "krylov_loops.hpp"

#include <cstdio>
#include <string>

using namespace spal;

namespace {

const char *const kVecNames[] = {"V_DOT", "V_DOT2", "V_INIT", "V_COPY_DOT", "V_CG_XR", "V_CG_P", "V_BI_P", "V_BI_S", "V_BI_HALF", "V_BI_XR"};
const char *const kFinNames[] = {"F_STORE", "F_INIT", "F_RZ", "F_ALPHA_CG", "F_TEST_CG", "F_BETA", "F_RHO", "F_ALPHA_BI", "F_HALF", "F_OMEGA", "F_TEST_BI"};
const char *const kCgWork[] = {"r", "q", "p", "z"};
const char *const kBiWork[] = {"r", "q", "p", "rhat", "v", "t", "ph", "sh"};

struct Recorder {
    bool cg = true, pre = false;
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
    const char *work(int i) const {
        if (i < 0 || i >= (cg ? 4 : 8) || (!pre && (cg ? i == 3 : i >= 6))) return "NO-SUCH-VECTOR";
        return cg ? kCgWork[i] : kBiWork[i];
    }
    bool preconditioned() const { return pre; }
    int mul(const char *in, const char *out) { return say(std::string("mul(") + in + "," + out + ")"); }
    int prec(const char *in, const char *out) { return say(std::string("prec(") + in + "," + out + ")"); }
    template <int OP>
    int v(const char *a, const char *b, const char *c, const char *d, const char *x, const char *y) {
        return say(std::string(kVecNames[OP]) + "(" + a + "," + b + "," + c + "," + d + "," + x + "," + y + ")");
    }
    template <int OP>
    int f(int unpreconditioned = 0) {
        return say(std::string(kFinNames[OP]) + "(" + std::to_string(unpreconditioned) + ")");
    }
    int copy(const char *dst, const char *src) { return say(std::string("copy(") + dst + "," + src + ")"); }
    int zero(const char *dst) { return say(std::string("zero(") + dst + ")"); }
    int poll() {
        ++npolls;
        return say("poll");
    }
    bool all_stopped() const { return stop_at_poll && npolls >= stop_at_poll; }
    uint64_t polls() const { return npolls; }
};

void loop(const char *name, bool cg, bool pre, uint64_t maxit, uint64_t check_every, uint64_t stop_at_poll = 0,
          uint64_t fail_at = 0) {
    Recorder r;
    r.cg = cg;
    r.pre = pre;
    r.stop_at_poll = stop_at_poll;
    r.fail_at = fail_at;
    const int status = cg ? cg_loop(r, maxit, check_every) : bicgstab_loop(r, maxit, check_every);
    printf("%s: %d | %s\n", name, status, r.trace.c_str());
}

}  // namespace

int main() {
    {
        Recorder r;
        const int status = krylov_start(r);
        printf("start: %d | %s\n", status, r.trace.c_str());
    }
    for (int cg = 1; cg >= 0; --cg) {
        const std::string m = cg ? "cg" : "bicgstab";
        loop((m + "_plain").c_str(), cg, false, 2, 2);
        loop((m + "_pre").c_str(), cg, true, 2, 2);
        loop((m + "_0_8").c_str(), cg, false, 0, 8);
        loop((m + "_5_2").c_str(), cg, false, 5, 2);
        loop((m + "_5_8").c_str(), cg, false, 5, 8);
        loop((m + "_40_1_stop3").c_str(), cg, false, 40, 1, 3);
        loop((m + "_fail6").c_str(), cg, false, 5, 2, 0, 6);
    }
    return 0;
}

// wide_plan_check.cpp -- stand-alone host check of the wide path's plan arithmetic (hk_pcond_plan.h, hk_wide_host.h):
// hk_pcond's LDS carve as pc_plan states it, the two bounds on d_cond_DCtd's integer bookkeeping, and make_layout's
// per-stage offsets.  No device work: what the headers expect from other translation units is defined here, and the
// launcher is never called.  tests/test_wide_plan_host.py compiles this with the address and undefined-behaviour
// sanitizers and runs it.
#include "../../hpmpc_amd/csrc/hk_pcond_plan.h"

thread_local int g_err = 0;
thread_local DevCtx g_dev;
extern "C" void hk_set_error(int code, const char*) { g_err = code; }
extern "C" int hk_wide_launch(int, const void*, int, int, hipStream_t) { abort(); }

static int failures = 0;
#define CHECK(cond, ...)                      \
    do {                                      \
        if (!(cond)) {                        \
            failures++;                       \
            printf("FAIL %s: ", #cond);       \
            printf(__VA_ARGS__);              \
            printf("\n");                     \
        }                                     \
    } while (0)

// One block (N2 = 1) of T stages: nx_0 = 0, then nx; nu on every stage of the block; idxb = inputs then the first
// `boxed` states, on every stage (stage 0 has no state, the terminal stage no input).
struct Shape {
    int T;
    std::vector<int> nx, nu, nb, ng;
    std::vector<std::vector<int>> idx;
    std::vector<const int*> idxp;
    Shape(int nxv, int nuv, int T_, int boxed) : T(T_), nx(T_ + 1, nxv), nu(T_ + 1, nuv), nb(T_ + 1), ng(T_ + 1, 0) {
        nx[0] = 0;
        nu[T] = 0;
        idx.resize(T + 1);
        for (int k = 0; k <= T; k++) {
            for (int l = 0; l < nu[k]; l++) idx[k].push_back(l);
            for (int l = 0; l < (k > 0 ? boxed : 0); l++) idx[k].push_back(nu[k] + l);
            nb[k] = (int)idx[k].size();
            idxp.push_back(idx[k].data());
        }
    }
    bool plan(PcPlan& P) const { return pc_plan(P, T, nx.data(), nu.data(), nb.data(), idxp.data(), ng.data(), 1); }
};

static void check_plan(const PcPlan& P, int nxv, int nuv, int T, int boxed) {
    const long long bk = 6LL * T + 2LL * P.ng2[0];
    CHECK(P.ng2[0] == (T - 1) * boxed, "nx %d nu %d T %d boxed %d: ng2 %d", nxv, nuv, T, boxed, P.ng2[0]);
    CHECK(P.offP <= P.offX && P.offX <= P.offB && P.offB == P.offW && P.offW <= P.offGA && P.offGA <= P.offST &&
              P.offST <= P.offU && P.offU <= P.offGT && P.offGT < P.pc_lds,
          "nx %d nu %d T %d boxed %d: carve %d %d %d %d %d %d %d %d lds %d", nxv, nuv, T, boxed, P.offP, P.offX, P.offB,
          P.offW, P.offGA, P.offST, P.offU, P.offGT, P.pc_lds);
    CHECK(bk <= 2LL * P.offST, "nx %d nu %d T %d boxed %d: bookkeeping %lld ints over the stage table at %d", nxv, nuv,
          T, boxed, bk, 2 * P.offST);
    CHECK(!P.pc_dm_ok || bk <= 2LL * P.offB, "nx %d nu %d T %d boxed %d: dm with bookkeeping %lld ints over offB at %d",
          nxv, nuv, T, boxed, bk, 2 * P.offB);
}

// a named case: accepted, with the bookkeeping, 2 offB and the dm route worked out by hand from pc_plan's formulas
static void named(int nxv, int nuv, int T, int boxed, long long bk, int offB2, bool dm) {
    PcPlan P;
    const bool ok = Shape(nxv, nuv, T, boxed).plan(P);
    CHECK(ok, "nx %d nu %d T %d boxed %d refused", nxv, nuv, T, boxed);
    if (!ok) return;
    check_plan(P, nxv, nuv, T, boxed);
    CHECK(6LL * T + 2LL * P.ng2[0] == bk && 2 * P.offB == offB2 && P.pc_dm_ok == dm,
          "nx %d nu %d T %d boxed %d: bookkeeping %lld (want %lld), 2 offB %d (want %d), dm %d (want %d)", nxv, nuv, T,
          boxed, 6LL * T + 2LL * P.ng2[0], bk, 2 * P.offB, offB2, (int)P.pc_dm_ok, (int)dm);
}

// make_layout's stage offsets against the running sums of the lib4 sizes, for time-varying stage sizes
static void check_layout() {
    const int N = 13;
    const int nx[N + 1] = {0, 5, 9, 24, 7, 12, 12, 3, 16, 10, 8, 8, 20, 6};
    const int nu[N + 1] = {3, 2, 6, 1, 4, 4, 5, 2, 3, 6, 2, 3, 1, 0};
    const int nb[N + 1] = {2, 4, 8, 3, 5, 9, 7, 2, 6, 8, 4, 5, 9, 3};
    const int ng[N + 1] = {0};
    const WLayout L = make_layout(N, nx, nu, nb, ng);
    auto r = [](int n, int m) { return (n + m - 1) / m * m; };
    long long oB = 0, oR = 0, oL = 0, oU = 0, oP = 0, oD = 0, oI = 0;
    for (int k = 0; k <= N; k++) {
        const WideStage& s = L.st[k];
        const int nux = nu[k] + nx[k], nx1 = k < N ? nx[k + 1] : 0;
        CHECK(s.nu == nu[k] && s.nx == nx[k] && s.nx1 == nx1 && s.nu1 == (k + 1 < N ? nu[k + 1] : 0), "stage %d sizes", k);
        CHECK(s.sdB == r(nx1, 2) && s.sdR == r(nux, 2) && s.nb == nb[k] && s.pnb == r(nb[k], 4) && s.ng == 0 && s.sdG == 0,
              "stage %d strides", k);
        CHECK(s.oB == oB && s.oR == oR && s.oL == oL && s.oU == oU && s.oP == oP && s.oD == oD && s.oI == oI && s.oG == 0,
              "stage %d offsets: %d %d %d %d %d %d %d, want %lld %lld %lld %lld %lld %lld %lld", k, s.oB, s.oR, s.oL, s.oU,
              s.oP, s.oD, s.oI, oB, oR, oL, oU, oP, oD, oI);
        CHECK(len_BAbt(s) == (size_t)r(nux + 1, 4) * r(nx1, 2) && len_RSQ(s) == (size_t)r(nux + 1, 4) * r(nux, 2) &&
                  len_cvec(s) == 2 * r(nb[k], 4), "stage %d lengths", k);
        if (k < N) oB += r(nux + 1, 4) * r(nx1, 2);
        oR += r(nux + 1, 4) * r(nux, 2);
        oL = r(oL + nux * (nux + 1) - nux * (nux - 1) / 2 + nux, 8);  // packed lower columns of nux+1 rows, then 1/diag
        oU += r(nux + 1, 8);
        oP += r(nx1 + 1, 8);
        oD += 2 * r(nb[k], 4);
        oI += nb[k];
    }
    CHECK(L.nB == oB && L.nR == oR && L.nL == oL && L.nU == oU && L.nP == oP && L.nD == oD && L.nI == oI && L.nG == 1,
          "layout totals");
    CHECK(L.fits && !L.any_ng, "layout flags");
}

int main() {
    int accepted = 0, refused = 0;
    for (int nxv : {4, 8, 12, 24})
        for (int nuv : {0, 1, 4, 6})
            for (int T : {2, 10, 24, 50, 100})
                for (int boxed : {0, nxv / 2, nxv}) {
                    PcPlan P;
                    if (!Shape(nxv, nuv, T, boxed).plan(P)) {
                        refused++;
                        continue;
                    }
                    accepted++;
                    check_plan(P, nxv, nuv, T, boxed);
                }
    CHECK(accepted > 0 && refused > 0, "sweep: %d accepted, %d refused", accepted, refused);
    named(24, 6, 10, 12, 276, 3480, true);   // the benchmark block: the deferred cross terms stay on
    named(8, 1, 24, 8, 512, 424, false);     // a long block, every state boxed: the reference's order
    named(12, 4, 50, 12, 1476, 1088, false);
    check_layout();
    printf("wide_plan_check: %d plans accepted, %d refused, %d failures\n", accepted, refused, failures);
    return failures ? 1 : 0;
}

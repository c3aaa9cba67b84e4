// hpmpc_capi.cpp -- host side of libhpmpc_mi355x.so, the part every other host file builds on: the thread's
// error code and device context (hk_host.h), the plan with its caller-layout tables (hk_plan.h), the version and
// debug hooks, and the batched device API (ipm_batch, ipm_solo, ipm_pass, ipm_batch_profiled, ric_*_batch).  The
// problem queue is in hpmpc_capi_queue.cpp, the reference-named single-problem entry points in
// hpmpc_capi_dropin.cpp (hard constraints) and hpmpc_capi_soft.cpp (soft constraints).  Every call runs on the GPU
// through the kernels in hpmpc_kernels.hip; there is no CPU fallback.
#include <cstdlib>

#include "hk_launch_guard.h"
#include "hk_plan.h"

thread_local int g_err = 0;
thread_local DevCtx g_dev;

extern "C" void hk_set_error(int code, const char* what) {
    g_err = code;
    if (code) fprintf(stderr, "[hpmpc_mi355x] %s (code %d)\n", what, code);
}

// d_back_ric_rec_sv_tv_res runs the two-wave kernel (hk_ric2.hip: the tile recursion on one wave, fetch / row half /
// stores on the other) when the library is the ric2 build variant (hpmpc_amd.build.build_ric2, -DHK_RIC2),
// HPMPC_MI355X_RIC_WAVES=2 asks for it and its launch guard accepts the launch (HK_LAUNCH_REFUSED,
// hk_launch_guard.h).  The product library has the one-wave kernel only: it measured faster at every batch (DESIGN.md
// §4, round 5).  Every other entry point is hk_launch's.
int launch(int which, const KArgs* a, int count, hipStream_t s) {
#ifdef HK_RIC2
    if (which == K_SV) {
        const char* e = getenv("HPMPC_MI355X_RIC_WAVES");
        if (e && e[0] == '2') {
            const int r = hk_launch_ric2(which, a, count, s);
            if (r != HK_LAUNCH_REFUSED) return r;
        }
    }
#endif
    return hk_launch(which, a, count, s);
}

// ------------------------------------------------------------------------------------------------
// Plan: stage tables shared by every problem of a batch.
// ------------------------------------------------------------------------------------------------
bool plan_supported(int N, const int* nx, const int* nu, const int* nb, const int* const* idxb, const int* ng,
                    const char** why) {
    // the tile kernels stage the plan's tables in LDS (lds_table_bytes, hk_ipm_body.h: Scratch + per stage StageInfo,
    // tile / slot tables and the certificate bound), within the 160 KiB one workgroup may use
    if (LDS_FIXED + (long long)LDS_PER_STAGE * (N + 1) > 160 * 1024) {
        *why = "horizon beyond the LDS stage tables of the tile kernels (N <= 1571)";
        return false;
    }
    for (int k = 0; k <= N; k++) {
        const int u = k < N ? nu[k] : 0;
        if (ng[k] < 0 || rup(nb[k], 4) + rup(ng[k], 4) > 16) {
            *why = "round_up(nb[k],4) + round_up(ng[k],4) must be <= 16 (one 32-slot constraint vector per stage)";
            return false;
        }
        if (u < 0 || nx[k] < 0 || u + nx[k] > 16 || rup(u, 4) + nx[k] > 16) {
            *why = "stage size beyond the 16-wide tile (nu+nx <= 16, round_up(nu,4)+nx <= 16)";
            return false;
        }
        if (nb[k] < 0 || nb[k] > u + nx[k]) {
            *why = "nb[k] > nu[k]+nx[k]";
            return false;
        }
        if (idxb) {  // box indices: in range and distinct (one box per variable)
            unsigned seen = 0;
            for (int j = 0; j < nb[k]; j++) {
                const int v = idxb[k][j];
                if (v < 0 || v >= u + nx[k] || (seen >> v & 1u)) {
                    *why = "idxb[k] must hold distinct variable indices in [0, nu[k]+nx[k])";
                    return false;
                }
                seen |= 1u << v;
            }
        }
    }
    if (N < 1) {
        *why = "N must be >= 1";
        return false;
    }
    return true;
}

// The device stage table for the given stage offsets and shared-block flags (StageInfo r0 bits 1 / 2: the block of
// stage k sits at the batch's base + offset for every problem): the plan's default table when they are the packed
// defaults, else the table of that layout (uploaded on first use, cached for the plan's lifetime).
static const void* plan_stage_table(const hpmpc_mi355x_plan* P, const long long* offB, const long long* offR,
                                    const unsigned char* shB = nullptr, const unsigned char* shR = nullptr) {
    const int N = P->N;
    std::vector<StageInfoH> st = P->st;
    for (int k = 0; k <= N; k++) {
        st[k].oB = k < N ? (int)offB[k] : 0;
        st[k].oR = (int)offR[k];
        st[k].r0 = (P->st[k].r0 & 1) | ((shB && k < N && shB[k]) ? 2 : 0) | ((shR && shR[k]) ? 4 : 0);
    }
    const size_t bytes = sizeof(StageInfoH) * (N + 1);
    if (!memcmp(st.data(), P->st.data(), bytes)) return P->d_st.get();
    std::lock_guard<std::mutex> lock(P->ltabs_mu);
    for (const auto& t : P->ltabs)
        if (!memcmp(st.data(), t.st.data(), bytes)) return t.d.get();
    // each distinct layout keeps a device table (and its first use a synchronous upload) until the plan is destroyed:
    // a caller whose offsets change from call to call would grow it without bound, so the cache is capped
    constexpr size_t kMaxLayouts = 64;
    if (P->ltabs.size() >= kMaxLayouts) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "more than 64 distinct stage layouts on one plan (create a plan per layout "
                                           "family, or keep the offsets fixed)");
        return nullptr;
    }
    DevTable<StageInfoH> d;
    if (!d.upload(st, "layout stage table")) return nullptr;
    P->ltabs.push_back({std::move(st), std::move(d)});
    return P->ltabs.back().d.get();
}

extern "C" hpmpc_mi355x_plan* hpmpc_mi355x_plan_create(int N, const int* nx, const int* nu, const int* nb,
                                                       const int* const* idxb, const int* ng) {
    const char* why = nullptr;
    if (!plan_supported(N, nx, nu, nb, idxb, ng, &why)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, why);
        return nullptr;
    }
    auto* P = new hpmpc_mi355x_plan();
    P->N = N;
    P->nx.assign(nx, nx + N + 1);
    P->nu.assign(nu, nu + N + 1);
    P->nu[N] = 0;
    P->nb.assign(nb, nb + N + 1);
    P->ng.assign(ng, ng + N + 1);
    P->idxb.resize(N + 1);
    P->st.resize(N + 1);
    P->tileslot.assign((N + 1) * 16, -1);
    P->slotvar.assign((N + 1) * 16, 0);
    P->offB.resize(N);
    P->offR.resize(N + 1);
    P->offG.resize(N + 1);
    for (int k = 0; k <= N; k++) {
        StageInfoH& s = P->st[k];
        s.nu = P->nu[k];
        s.nx = nx[k];
        s.nb = nb[k];
        s.ng = ng[k];
        s.xo = rup(s.nu, 4);
        s.nx1 = k < N ? nx[k + 1] : 0;
        s.nu1 = k + 1 < N ? P->nu[k + 1] : 0;
        s.xo1 = rup(s.nu1, 4);
        s.sdB = rup(s.nx1, NCL);
        s.sdR = rup(s.nu + s.nx, NCL);
        s.pnb = rup(nb[k], BS);
        s.oD = k * V32;
        s.r0 = 0;
        s.oG = (int)P->packG;
        P->offG[k] = P->packG;
        if (ng[k] > 0) P->packG += (long long)rup(s.nu + s.nx, BS) * rup(ng[k], NCL);
        P->nbt += ng[k];
        P->ngt += ng[k];
        const int nux = s.nu + s.nx;
        if (k < N) {
            P->offB[k] = P->packB;
            P->packB += (long long)rup(nux + 1, BS) * s.sdB;
        }
        P->offR[k] = P->packR;
        P->packR += (long long)rup(nux + 1, BS) * s.sdR;
        // idxb[k] is read only for a stage with boxes: callers without boxes may pass idxb = NULL (the reference's
        // test_d_ric_mpc.c does), exactly as the reference never touches it there
        if (nb[k] > 0) P->idxb[k].assign(idxb[k], idxb[k] + nb[k]);
        P->nbt += nb[k];
        for (int l = 0; l < nb[k]; l++) {
            const int v = idxb[k][l];
            const int t = v < s.nu ? v : s.xo + (v - s.nu);
            P->tileslot[k * 16 + t] = (signed char)l;
            P->slotvar[k * 16 + l] = (signed char)v;
        }
    }
    // Inner stages of one compiled class run the constant-shape kernel path (StageInfo.r0 = 1).
    if (N >= 3) {
        const int nuc = P->nu[1], nxc = nx[1];
        P->fixcls = hk_fixcls(nuc, nxc);
        if (P->fixcls)
            for (int k = 1; k <= N - 2; k++)
                P->st[k].r0 = (P->nu[k] == nuc && nx[k] == nxc && P->nu[k + 1] == nuc && nx[k + 1] == nxc &&
                               ng[k] == 0)
                                  ? 1
                                  : 0;
    }
    for (int k = 0; k <= N; k++) {  // the packed default layout
        P->st[k].oB = k < N ? (int)P->offB[k] : 0;
        P->st[k].oR = (int)P->offR[k];
    }
    if (!P->d_st.upload(P->st, "plan tables") || !P->d_tileslot.upload(P->tileslot, "plan tables") ||
        !P->d_slotvar.upload(P->slotvar, "plan tables")) {
        delete P;
        return nullptr;
    }
    g_err = 0;
    return P;
}

extern "C" void hpmpc_mi355x_plan_destroy(hpmpc_mi355x_plan* P) { delete P; }

void idxb_table(int N, const int* nb, const int* const* idxb, int* out) {
    for (int k = 0; k <= N; k++)
        for (int l = 0; l < nb[k]; l++) out[k * 16 + l] = idxb[k][l];
}

extern "C" long long hpmpc_mi355x_ws_doubles(const hpmpc_mi355x_plan* P) { return P ? ws_doubles(P->N) : 0; }

extern "C" int hpmpc_mi355x_last_error(void) { return g_err; }

// Diagnostic builds (-DHK_STAMPS, build.py build_stamps) record s_memtime stamps of problem 0 into this device
// buffer; only that build exports the setter (tools/stamps*.py load it through HPMPC_MI355X_LIB).
static unsigned long long* g_dbg_buf = nullptr;
#ifdef HK_STAMPS
extern "C" __attribute__((visibility("default"))) void hpmpc_mi355x_debug_buffer(void* dev_ptr) {
    g_dbg_buf = (unsigned long long*)dev_ptr;
}
#endif

extern "C" const char* hpmpc_mi355x_version(void) {
    return "hpmpc_mi355x 0.1 gfx950 (wave-per-problem, f64 MFMA 16x16x4 stage contractions)";
}

bool range_ok(const void* plan, int nprob, int p0, int count, const char* who) {
    if (plan && nprob > 0 && p0 >= 0 && count >= 0 && (long long)p0 + count <= nprob) return true;
    char msg[128];
    snprintf(msg, sizeof msg, "%s: plan or problem range", who);
    hk_set_error(HPMPC_MI355X_EUNSUPPORTED, msg);
    return false;
}

int null_array(const char* who) {
    char msg[128];
    snprintf(msg, sizeof msg, "%s: a required array is null", who);
    hk_set_error(HPMPC_MI355X_EUNSUPPORTED, msg);
    return g_err;
}

int launch_error(int e, const char* what) {
    hk_set_error(e == HK_LAUNCH_REFUSED ? HPMPC_MI355X_EUNSUPPORTED : HPMPC_MI355X_EHIP, what);
    return g_err;
}

bool batch_args(KArgs& a, const hpmpc_mi355x_plan* P, const hpmpc_mi355x_layout* lay, int nprob, int p0,
                DctPolicy policy, const double* DCt) {
    if (!P) {
        g_err = HPMPC_MI355X_EUNSUPPORTED;
        return false;
    }
    if (policy == DCT_NONE && P->ngt) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "batched entry points: general constraints (ng > 0) need the "
                                           "reference-named entry points");
        return false;
    }
    memset(&a, 0, sizeof a);
    a.N = P->N;
    a.nprob = nprob;
    a.p0 = p0;
    a.st = P->d_st.get();
    a.tileslot = P->d_tileslot.get();
    a.slotvar = P->d_slotvar.get();
    if (lay && lay->BAbt_off && lay->RSQrq_off) {
        a.st = plan_stage_table(P, lay->BAbt_off, lay->RSQrq_off, lay->BAbt_shared, lay->RSQrq_shared);
        if (!a.st) return false;
    }
    a.sB = lay ? lay->BAbt_stride : P->packB;
    a.sR = lay ? lay->RSQrq_stride : P->packR;
    a.DCt = P->ngt ? DCt : nullptr;
    a.sV16 = (long long)(P->N + 1) * V16;
    a.sV32 = (long long)(P->N + 1) * V32;
    a.sW = ws_doubles(P->N);
    a.fixcls = P->fixcls;
    a.nbt = P->nbt;
    a.ngt = P->ngt;
    a.sG = P->packG;
    a.dbg = g_dbg_buf;
    return true;
}

// The calling thread's plan cache of the host-buffer entry points (hpmpc_capi_dropin.cpp, hpmpc_capi_soft.cpp).
hpmpc_mi355x_plan* thread_plan(int N, const int* nx, const int* nu, const int* nb, int** idxb, const int* ng) {
    struct Cache {
        hpmpc_mi355x_plan* plan = nullptr;
        std::vector<int> key;
        ~Cache() {
            if (plan) hpmpc_mi355x_plan_destroy(plan);
        }
    };
    thread_local Cache c;
    std::vector<int> k;
    k.push_back(N);
    for (int i = 0; i <= N; i++) {
        k.push_back(nx[i]);
        k.push_back(i < N ? nu[i] : 0);
        k.push_back(nb[i]);
        k.push_back(ng[i]);
        for (int l = 0; l < nb[i]; l++) k.push_back(idxb[i][l]);
    }
    if (c.plan && k == c.key) return c.plan;
    if (c.plan) hpmpc_mi355x_plan_destroy(c.plan);
    c.plan = hpmpc_mi355x_plan_create(N, nx, nu, nb, idxb, ng);
    c.key = c.plan ? k : std::vector<int>();
    return c.plan;
}

// The IPM fields of an argument block whose plan tables and layout (st, sB, sR, and DCt / sG for general
// constraints) are set, then the launch: the body of every batched IPM entry point, hpmpc_mi355x_ocp_ipm_batch
// (hpmpc_capi_ocp.cpp) included.
int ipm_run(KArgs& a, int count, const double* BAbt, const double* RSQrq, const double* d, double* ux, double* pi,
            double* lam, double* t, double* ws, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
            int compute_mult, int* kk, int* ret, double* stat, int which, void* stream) {
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.d = d;
    a.ux = ux;
    a.pi = pi;
    a.lam = lam;
    a.t = t;
    a.ws = ws;
    a.k_max = k_max;
    a.mu0 = mu0;
    a.mu_tol = mu_tol;
    a.alpha_min = alpha_min;
    a.warm_start = warm_start;
    a.compute_mult = compute_mult;
    a.kk = kk;
    a.ret = ret;
    a.stat = stat;
    if (const int e = hk_launch(which, &a, count, (hipStream_t)stream)) return launch_error(e, "hk_ipm launch failed");
    return g_err = 0;
}

namespace {

int ipm_launch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob, int p0, int count,
               const double* BAbt, const double* RSQrq, const double* d, double* ux, double* pi, double* lam,
               double* t, double* ws, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
               int compute_mult, int* kk, int* ret, double* stat, int which, void* stream) {
    KArgs a;
    if (!batch_args(a, plan, lay, nprob, p0, DCT_NONE)) return g_err;
    return ipm_run(a, count, BAbt, RSQrq, d, ux, pi, lam, t, ws, k_max, mu0, mu_tol, alpha_min, warm_start,
                   compute_mult, kk, ret, stat, which, stream);
}

// hipEvents owned by one API call.  The destructor first waits for every event recorded on them.
struct CallEvents {
    std::vector<hipEvent_t> e;
    bool create(int n) {
        e.reserve(n);
        for (int i = 0; i < n; i++) {
            hipEvent_t x;
            if (!hip_ok(hipEventCreate(&x), "event create")) return false;
            e.push_back(x);
        }
        return true;
    }
    hipEvent_t& operator[](size_t i) { return e[i]; }
    ~CallEvents() {
        for (hipEvent_t x : e) {
            (void)hipEventSynchronize(x);
            (void)hipEventDestroy(x);
        }
    }
};

}  // namespace

extern "C" int hpmpc_mi355x_ipm_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                      int p0, int count, const double* BAbt, const double* RSQrq, const double* d,
                                      double* ux, double* pi, double* lam, double* t, double* ws, int k_max,
                                      double mu0, double mu_tol, double alpha_min, int warm_start, int compute_mult,
                                      int* kk, int* ret, double* stat, void* stream) {
    return ipm_launch(plan, lay, nprob, p0, count, BAbt, RSQrq, d, ux, pi, lam, t, ws, k_max, mu0, mu_tol, alpha_min,
                      warm_start, compute_mult, kk, ret, stat, K_IPM, stream);
}

extern "C" int hpmpc_mi355x_ipm_solo(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob, int p0,
                                     int count, const double* BAbt, const double* RSQrq, const double* d, double* ux,
                                     double* pi, double* lam, double* t, double* ws, int k_max, double mu0,
                                     double mu_tol, double alpha_min, int warm_start, int compute_mult, int* kk,
                                     int* ret, double* stat, void* stream) {
    return ipm_launch(plan, lay, nprob, p0, count, BAbt, RSQrq, d, ux, pi, lam, t, ws, k_max, mu0, mu_tol, alpha_min,
                      warm_start, compute_mult, kk, ret, stat, K_SOLO, stream);
}

extern "C" int hpmpc_mi355x_ipm_batch_profiled(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay,
                                               int nprob, int p0, int count, const double* BAbt, const double* RSQrq,
                                               const double* d, double* ux, double* pi, double* lam, double* t,
                                               double* ws, int k_max, double mu0, double mu_tol, double alpha_min,
                                               int warm_start, int compute_mult, int* kk, int* ret, double* stat,
                                               double* pass_ms, void* stream) {
    // the same launch sequence as hpmpc_mi355x_ipm_batch, with a hipEvent pair around every pass kernel
    // (events are per call: they belong to the current device, and nothing outlives the call)
    const int npass = 1 + 4 * (k_max > 0 ? k_max : 0);
    CallEvents ev;
    if (!ev.create(2 * npass)) return g_err;
    hipStream_t st = (hipStream_t)stream;
    for (int i = 0; i < npass; i++) {
        const int which = i == 0 ? K_PASS_INIT : K_PASS_FACT + (i - 1) % 4;
        if (!hip_ok(hipEventRecord(ev[2 * i], st), "event record")) return g_err;
        int rc = ipm_launch(plan, lay, nprob, p0, count, BAbt, RSQrq, d, ux, pi, lam, t, ws, k_max, mu0, mu_tol,
                            alpha_min, warm_start, compute_mult, kk, ret, stat, which, stream);
        if (rc) return rc;
        if (!hip_ok(hipEventRecord(ev[2 * i + 1], st), "event record")) return g_err;
    }
    if (!hip_ok(hipStreamSynchronize(st), "sync")) return g_err;
    for (int p = 0; p < 5; p++) pass_ms[p] = 0.0;
    for (int i = 0; i < npass; i++) {
        float ms = 0.f;
        if (!hip_ok(hipEventElapsedTime(&ms, ev[2 * i], ev[2 * i + 1]), "event time")) return g_err;
        pass_ms[i == 0 ? 0 : 1 + (i - 1) % 4] += ms;
    }
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ipm_pass(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                     int p0, int count, const double* BAbt, const double* RSQrq, const double* d,
                                     double* ux, double* pi, double* lam, double* t, double* ws, int k_max,
                                     double mu0, double mu_tol, double alpha_min, int warm_start, int compute_mult,
                                     int* kk, int* ret, double* stat, int pass, void* stream) {
    if (pass < 0 || pass > 4) return g_err = HPMPC_MI355X_EUNSUPPORTED;
    return ipm_launch(plan, lay, nprob, p0, count, BAbt, RSQrq, d, ux, pi, lam, t, ws, k_max, mu0, mu_tol, alpha_min,
                      warm_start, compute_mult, kk, ret, stat, K_PASS_INIT + pass, stream);
}

extern "C" int hpmpc_mi355x_ric_sv_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                         int p0, int count, const double* BAbt, const double* RSQrq, double* ux,
                                         double* pi, double* ws, int compute_pi, int compute_Pb, double* Pb,
                                         void* stream) {
    KArgs a;
    if (!batch_args(a, plan, lay, nprob, p0, DCT_NONE)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ux = ux;
    a.pi = pi;
    a.ws = ws;
    a.compute_pi = compute_pi;
    a.compute_Pb = compute_Pb && Pb;
    a.vPb = Pb;
    if (const int e = launch(K_SV, &a, count, (hipStream_t)stream)) return launch_error(e, "hk_ric_sv launch failed");
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ric_trf_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                          int p0, int count, const double* BAbt, const double* RSQrq, double* ws,
                                          void* stream) {
    KArgs a;
    if (!batch_args(a, plan, lay, nprob, p0, DCT_NONE)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ws = ws;
    if (const int e = hk_launch(K_TRF, &a, count, (hipStream_t)stream))
        return launch_error(e, "hk_ric_trf launch failed");
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ric_trs_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                          int p0, int count, const double* BAbt, const double* RSQrq, const double* b,
                                          const double* q, double* ux, double* pi, double* ws, int compute_pi,
                                          int compute_Pb, double* Pb, void* stream) {
    KArgs a;
    if (!batch_args(a, plan, lay, nprob, p0, DCT_NONE)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.vb = b;
    a.vq = q;
    a.ux = ux;
    a.pi = pi;
    a.ws = ws;
    a.compute_pi = compute_pi;
    a.compute_Pb = compute_Pb;
    a.vPb = Pb;
    if (const int e = hk_launch(K_TRS, &a, count, (hipStream_t)stream))
        return launch_error(e, "hk_ric_trs launch failed");
    return g_err = 0;
}


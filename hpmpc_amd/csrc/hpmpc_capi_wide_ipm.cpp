// hpmpc_capi_wide_ipm.cpp -- host side of the IPM on wide stages (hk_wide_ipm.hip).
//
// hpmpc_capi_dropin.cpp routes the reference-named IPM entry points here when a problem does not fit the 16-wide
// register tile (nu+nx > 16, round_up(nu,4)+nx > 16, or more than 16 box + general slots in a stage):
//   d_ip2_res_mpc_hard_tv, d_ip2_res_mpc_hard_tv_single_newton_step, d_kkt_solve_new_rhs_res_mpc_hard_tv,
//   d_res_res_mpc_hard_tv (mpc_solvers/d_ip2_res_hard.c, c99/d_res_ip_res_hard.c), and d_ip2_mpc_hard_tv,
//   d_kkt_solve_new_rhs_mpc_hard_tv, d_res_mpc_hard_tv (mpc_solvers/d_ip2_hard.c, d_res_ip_hard.c).
// Arguments are the reference's host lib4 buffers.  Each call stages them into a pinned arena, uploads it with
// one copy, runs ONE launch of hk_wide_ipm (the whole solve on the device) and copies the results back.
// `double_work_memory` holds this library's private work image (factor, IPM vectors, iterate backup), so the
// KKT re-solves find what the IPM left; its size is d_ip2_res_mpc_hard_tv_work_space_size_bytes.
#include "hk_wide_host.h"

namespace {
// the wide IPM's LDS: the Riccati carve, 8 doubles of reduction scratch, the DCt chunk-limit table ((N+1) x 8 ints
// and a flag, hk_wide_core.h)
inline int ipm_lds(const WLayout& L) { return L.lds + 8 + ((L.N + 1) * KC_STRIDE + 2) / 2; }
}  // namespace

namespace {

// The per-problem work image of the wide IPM (offsets in doubles).
struct WIpm {
    WLayout L;
    int oF, oDux, oDpi, oPb, oRq, oRb, oUb, oPib, oC[10];
    long long nIW;
    std::vector<WideCSlot> cs;
    std::vector<int> vbox;
    long long nbt = 0;  // sum(nb + ng)
};

WIpm make_ipm(int N, const int* nx, const int* nu, const int* nb, const int* ng) {
    WIpm W;
    W.L = make_layout(N, nx, nu, nb, ng);
    const WLayout& L = W.L;
    long long o = 0;
    auto take = [&](long long n) {
        const long long r = o;
        o += (n + 7) / 8 * 8;
        return (int)r;
    };
    W.oF = take(L.nL);
    W.oDux = take(L.nU);
    W.oDpi = take(L.nP);
    W.oPb = take(L.nP);
    W.oRq = take(L.nU);
    W.oRb = take(L.nP);
    W.oUb = take(L.nU);
    W.oPib = take(L.nP);
    for (int i = 0; i < 10; i++) W.oC[i] = take(L.nD);
    W.nIW = o;
    for (int k = 0; k <= N; k++) W.nbt += nb[k] + ng[k];
    return W;
}

// constraint slots and the variable -> box map (needs idxb)
void fill_slots(WIpm& W, int N, int** idxb) {
    const WLayout& L = W.L;
    W.cs.clear();
    W.vbox.assign(L.nU, -1);
    for (int k = 0; k <= N; k++) {
        const WideStage& s = L.st[k];
        const int png = rup(s.ng, BS);
        for (int l = 0; l < s.nb; l++) {
            WideCSlot c;
            c.lo = s.oD + l;
            c.up = s.oD + s.pnb + l;
            c.q = s.oD + l;
            c.var = s.oU + idxb[k][l];
            c.g = 0;
            W.cs.push_back(c);
            W.vbox[s.oU + idxb[k][l]] = c.lo;
        }
        for (int g = 0; g < s.ng; g++) {
            WideCSlot c;
            c.lo = s.oD + 2 * s.pnb + g;
            c.up = s.oD + 2 * s.pnb + png + g;
            c.q = s.oD + s.pnb + g;
            c.var = -1 - k;
            c.g = g;
            W.cs.push_back(c);
        }
    }
}

// sizes the wide IPM serves: any nb <= nu+nx with distinct indices, any ng, stage tiles within the kernel limits
bool ipm_check(const WIpm& W, int N, const int* nx, const int* nu, const int* nb, int* const* idxb, const int* ng) {
    if (N < 1) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "N must be >= 1");
        return false;
    }
    for (int k = 0; k <= N; k++) {
        const int nux = (k < N ? nu[k] : 0) + nx[k];
        if (nb[k] < 0 || nb[k] > nux || ng[k] < 0 || nx[k] < 0 || (k < N && nu[k] < 0)) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "negative size or nb[k] > nu[k]+nx[k]");
            return false;
        }
        if (idxb) {
            std::vector<char> seen(nux > 0 ? nux : 1, 0);
            for (int l = 0; l < nb[k]; l++) {
                const int v = idxb[k][l];
                if (v < 0 || v >= nux || seen[v]) {
                    hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "idxb[k] must hold distinct variable indices in [0, nu[k]+nx[k])");
                    return false;
                }
                seen[v] = 1;
            }
        }
    }
    if (!W.L.fits || ipm_lds(W.L) > LDS_MAX_DOUBLES) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "wide stage beyond the kernel's tile limits (64 KiB LDS, nu+nx < 128, "
                                                "nx <= 64)");
        return false;
    }
    return true;
}

// Staging arena of one call.
struct IpmCtl {  // what the kernel leaves for the host: kk, the return code, mu (residual routines: in / out)
    int kk, ret;
    double mu, pad[6];
};
struct Stage {
    Slot<WideStage> st;
    Slot<WideCSlot> cs;
    Slot<int> vbox, idxb;
    Slot<double> B, R, G, d, ux, pi, lam, t, vb, vq, iw, stat;
    Slot<IpmCtl> ctl;
    size_t total;
};

Stage carve(const WIpm& W, int N, int k_max) {
    const WLayout& L = W.L;
    Carve c;
    Stage S;
    S.st = c.take<WideStage>(N + 1);
    S.cs = c.take<WideCSlot>(W.cs.size() + 1);
    S.vbox = c.take<int>(L.nU);
    S.idxb = c.take<int>(L.nI);
    S.B = c.take<double>(L.nB);
    S.R = c.take<double>(L.nR);
    S.G = c.take<double>(L.nG);
    S.d = c.take<double>(L.nD);
    S.ux = c.take<double>(L.nU);
    S.pi = c.take<double>(L.nP);
    S.lam = c.take<double>(L.nD);
    S.t = c.take<double>(L.nD);
    S.vb = c.take<double>(L.nP);
    S.vq = c.take<double>(L.nU);
    S.iw = c.take<double>(W.nIW);
    S.stat = c.take<double>(5 * (size_t)(k_max > 0 ? k_max : 1) + 8);
    S.ctl = c.take<IpmCtl>(1);
    S.total = c.o;
    return S;
}

// Everything in WideIpmArgs that follows from the work image, for problems [p0, ..) of nprob; the pointers are the
// caller's: the one-problem arena (stage) or a batch's device arrays (hpmpc_mi355x_wide_ipm_batch).
void ipm_args(const WIpm& W, int nprob, int p0, int k_max, WideIpmArgs& a) {
    const WLayout& L = W.L;
    memset(&a, 0, sizeof a);
    wide_args(L, nprob, p0, a.w);
    a.k_max = k_max;
    a.mu_scal = W.nbt ? 1.0 / (2.0 * (double)W.nbt) : 0.0;
    a.nbt2 = 2.0 * (double)W.nbt;
    a.ncs = (int)W.cs.size();
    a.nU = (int)L.nU;
    a.nP = (int)L.nP;
    a.sC = L.nD;
    a.sI = W.nIW;
    a.sS = 5LL * (k_max > 0 ? k_max : 1);
    a.oF = W.oF;
    a.oDux = W.oDux;
    a.oDpi = W.oDpi;
    a.oPb = W.oPb;
    a.oRq = W.oRq;
    a.oRb = W.oRb;
    a.oUb = W.oUb;
    a.oPib = W.oPib;
    int* oc[10] = {&a.oDlam, &a.oDt, &a.oTinv, &a.oLamt, &a.oRd, &a.oRm, &a.oTb, &a.oLb, &a.oQx, &a.oqx};
    for (int i = 0; i < 10; i++) *oc[i] = W.oC[i];
    a.offR = L.lds;
    a.offKC = L.lds + 8;
}

// one launch of hk_wide_ipm; 0, or the error code it set
int ipm_launch(const WIpm& W, const WideIpmArgs& a, int count, hipStream_t stream) {
    const int e = hk_wide_ipm_launch(&a, count, ipm_lds(W.L), stream);
    if (!e) return 0;
    char msg[96];
    snprintf(msg, sizeof msg, "hk_wide_ipm launch %s (%d)", e == -2 ? "refused: scratch / LDS beyond the limits" : "failed", e);
    const int code = e == -2 ? HPMPC_MI355X_EUNSUPPORTED : HPMPC_MI355X_EHIP;
    hk_set_error(code, msg);
    return code;
}

// stage the tables and the problem data (lib4 blocks, possibly aliased stage pointers) and point the one-problem
// argument block at the arena
void stage(const WIpm& W, const Stage& S, int k_max, int** idxb, double** pBAbt, double** pQ, double** pDCt, double** d,
           WideIpmArgs& a) {
    const WLayout& L = W.L;
    S.st.put(L.st);
    S.cs.put(W.cs);
    S.vbox.put(W.vbox);
    idxb_in(L, S.idxb.host(), idxb);
    BAbt_in(L, S.B.host(), pBAbt);
    RSQ_in(L, S.R.host(), pQ);
    DCt_in(L, S.G.host(), pDCt);
    cvec_in(L, S.d.host(), d);
    ipm_args(W, 1, 0, k_max, a);
    a.w.st = S.st.dev();
    a.w.BAbt = S.B.dev();
    a.w.RSQ = S.R.dev();
    a.w.DCt = S.G.dev();
    a.w.idxb = S.idxb.dev();
    a.cs = S.cs.dev();
    a.vbox = S.vbox.dev();
    a.d = S.d.dev();
    a.ux = S.ux.dev();
    a.pi = S.pi.dev();
    a.lam = S.lam.dev();
    a.t = S.t.dev();
    a.iw = S.iw.dev();
    a.stat = S.stat.dev();
    a.kk = &S.ctl.dev()->kk;
    a.ret = &S.ctl.dev()->ret;
    a.mu = &S.ctl.dev()->mu;
}

bool run(const WIpm& W, const Stage& S, const WideIpmArgs& a) {
    return g_dev.up(S.total) && !ipm_launch(W, a, 1, g_dev.stream) && g_dev.down(S.total);
}

}  // namespace

// bytes of the wide IPM's work image for these sizes (hpmpc_capi_dropin.cpp reports the larger of this and the tile
// path's image as d_ip2_res_mpc_hard_tv_work_space_size_bytes)
extern "C" long long hk_wide_ipm_bytes(int N, const int* nx, const int* nu, const int* nb, const int* ng) {
    return make_ipm(N, nx, nu, nb, ng).nIW * 8;
}

// d_ip2_res_mpc_hard_tv (mode WI_IPM_RES), its single-Newton variant (WI_NEWTON) and d_ip2_mpc_hard_tv
// (WI_IPM_P1) on wide stages.
extern "C" int hk_wide_ipm_entry(int mode, int* kk, int k_max, double mu0, double mu_tol, double alpha_min,
                                 int warm_start, double* stat, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng,
                                 double** pBAbt, double** pQ, double** pDCt, double** d, double** ux,
                                 int compute_mult, double** pi, double** lam, double** t, double* work, double** ux0,
                                 double** pi0, double** lam0, double** t0) {
    hk_set_error(0, nullptr);
    std::vector<int> nu(nu_N, nu_N + N + 1);
    nu[N] = 0;
    WIpm W = make_ipm(N, nx, nu.data(), nb, ng);
    const WLayout& L = W.L;
    if (!ipm_check(W, N, nx, nu.data(), nb, idxb, ng)) return HPMPC_MI355X_EUNSUPPORTED;
    if (mode == WI_NEWTON) {
        for (int k = 0; k <= N; k++)
            if (ng[k] > 0) {  // the reference stops here too (d_aux_ip_hard_lib4.c:197-208)
                hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "single Newton step with general constraints");
                return HPMPC_MI355X_EUNSUPPORTED;
            }
    }
    fill_slots(W, N, idxb);
    const Stage S = carve(W, N, k_max);
    if (!g_dev.ensure(S.total)) return HPMPC_MI355X_EHIP;
    WideIpmArgs a;
    stage(W, S, k_max, idxb, pBAbt, pQ, pDCt, d, a);
    if (mode == WI_NEWTON) {  // start iterate; lam0 / t0 as [lower (nb) | upper (nb)] (d_aux_ip_hard_lib4.c:153-213)
        uvec_in(L, S.ux.host(), ux0);
        pvec_in(L, S.pi.host(), pi0);
        for (int k = 0; k <= N; k++) {
            const WideStage& s = L.st[k];
            for (int l = 0; l < nb[k]; l++) {
                S.lam.host()[s.oD + l] = lam0[k][l];
                S.lam.host()[s.oD + s.pnb + l] = lam0[k][nb[k] + l];
                S.t.host()[s.oD + l] = t0[k][l];
                S.t.host()[s.oD + s.pnb + l] = t0[k][nb[k] + l];
            }
        }
    } else if (warm_start) {
        uvec_in(L, S.ux.host(), ux);
    }
    a.mode = mode;
    a.warm_start = warm_start;
    a.compute_mult = compute_mult;
    a.mu0 = mu0;
    a.mu_tol = mu_tol;
    a.alpha_min = alpha_min;
    if (!run(W, S, a)) return HPMPC_MI355X_EHIP;
    const IpmCtl& ctl = *S.ctl.host();
    *kk = ctl.kk;
    for (int i = 0; i < 5 * ctl.kk; i++) stat[i] = S.stat.host()[i];
    // d_ip2_mpc_hard_tv without constraints solves into its workspace only (d_ip2_hard.c:282-291)
    if (!(mode == WI_IPM_P1 && W.nbt == 0)) {
        uvec_out(L, S.ux.host(), ux);
        pvec_out(L, S.pi.host(), pi);
        cvec_out(L, S.lam.host(), lam);
        cvec_out(L, S.t.host(), t);
    }
    memcpy(work, S.iw.host(), W.nIW * sizeof(double));
    return ctl.ret;
}

// d_kkt_solve_new_rhs_res_mpc_hard_tv (p1 = 0: b / q / d) and d_kkt_solve_new_rhs_mpc_hard_tv (p1 = 1:
// r_A / r_H / r_C) over the work image the IPM left.
extern "C" void hk_wide_kkt_entry(int p1, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng, double** pBAbt,
                                  double** b, double** pQ, double** q, double** pDCt, double** d, double** ux,
                                  int compute_mult, double** pi, double** lam, double** t, double* work) {
    hk_set_error(0, nullptr);
    std::vector<int> nu(nu_N, nu_N + N + 1);
    nu[N] = 0;
    WIpm W = make_ipm(N, nx, nu.data(), nb, ng);
    const WLayout& L = W.L;
    if (!ipm_check(W, N, nx, nu.data(), nb, idxb, ng)) return;
    fill_slots(W, N, idxb);
    const Stage S = carve(W, N, 1);
    if (!g_dev.ensure(S.total)) return;
    WideIpmArgs a;
    stage(W, S, 0, idxb, pBAbt, pQ, pDCt, d, a);
    uvec_in(L, S.vq.host(), q);
    pvec_in(L, S.vb.host(), b);
    memcpy(S.iw.host(), work, W.nIW * sizeof(double));
    a.mode = p1 ? WI_KKT_P1 : WI_KKT_RES;
    a.compute_mult = compute_mult;
    a.vb = S.vb.dev();
    a.vq = S.vq.dev();
    if (!run(W, S, a)) return;
    uvec_out(L, S.ux.host(), ux);
    if (compute_mult || !p1) pvec_out(L, S.pi.host(), pi);
    cvec_out(L, S.lam.host(), lam);
    cvec_out(L, S.t.host(), t);
    if (p1) memcpy(work, S.iw.host(), W.nIW * sizeof(double));  // qx / Pb of the re-solve, as the reference leaves them
}

// d_res_res_mpc_hard_tv (plain = 0: r_q, r_b, r_d, r_m, mu) and d_res_mpc_hard_tv (plain = 1: r_q, r_b, r_d, mu).
extern "C" void hk_wide_res_entry(int plain, int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                  double** hb, double** hpQ, double** hq, double** hux, double** hpDCt, double** hd,
                                  double** hpi, double** hlam, double** ht, double** hrq, double** hrb, double** hrd,
                                  double** hrm, double* mu) {
    hk_set_error(0, nullptr);
    WIpm W = make_ipm(N, nx, nu, nb, ng);
    const WLayout& L = W.L;
    if (!ipm_check(W, N, nx, nu, nb, idxb, ng)) return;
    fill_slots(W, N, idxb);
    const Stage S = carve(W, N, 1);
    if (!g_dev.ensure(S.total)) return;
    WideIpmArgs a;
    stage(W, S, 0, idxb, hpBAbt, hpQ, hpDCt, hd, a);
    cvec_in(L, S.lam.host(), hlam);
    cvec_in(L, S.t.host(), ht);
    uvec_in(L, S.ux.host(), hux);
    pvec_in(L, S.pi.host(), hpi);
    uvec_in(L, S.vq.host(), hq);
    pvec_in(L, S.vb.host(), hb);
    S.ctl.host()->mu = *mu;  // unchanged without constraints (d_res_ip_res_hard.c:309-313)
    a.mode = plain ? WI_RES_PLAIN : WI_RES;
    a.vb = S.vb.dev();
    a.vq = S.vq.dev();
    if (!run(W, S, a)) return;
    const double* IW = S.iw.host();
    uvec_out(L, IW + W.oRq, hrq);
    pvec_out(L, IW + W.oRb, hrb);
    cvec_out(L, IW + W.oC[4], hrd);
    if (!plain) cvec_out(L, IW + W.oC[5], hrm);
    *mu = S.ctl.host()->mu;
}

// ------------------------------------------------------------------------------------------------
// Batched device API of the wide-stage IPM (include/hpmpc_mi355x.h, Part 2): many problems that share the
// stage sizes and box index sets, data resident in HBM, one workgroup per problem, one launch per batch.
// ------------------------------------------------------------------------------------------------
struct hpmpc_mi355x_wide_plan {
    WIpm W;
    int N = 0;
    DevTable<WideStage> d_st;
    DevTable<WideCSlot> d_cs;
    DevTable<int> d_vbox, d_idxb;
};

extern "C" void hpmpc_mi355x_wide_plan_destroy(hpmpc_mi355x_wide_plan* q) { delete q; }

extern "C" hpmpc_mi355x_wide_plan* hpmpc_mi355x_wide_plan_create(int N, const int* nx, const int* nu_in, const int* nb,
                                                                 const int* const* idxb, const int* ng) {
    hk_set_error(0, nullptr);
    std::vector<int> nu(nu_in, nu_in + N + 1);
    nu[N] = 0;
    auto* q = new hpmpc_mi355x_wide_plan();
    q->N = N;
    q->W = make_ipm(N, nx, nu.data(), nb, ng);
    int** ib = const_cast<int**>(idxb);
    if (!ipm_check(q->W, N, nx, nu.data(), nb, ib, ng)) {
        delete q;
        return nullptr;
    }
    fill_slots(q->W, N, ib);
    const WLayout& L = q->W.L;
    std::vector<int> hidx(L.nI, 0);
    idxb_in(L, hidx.data(), ib);
    std::vector<WideCSlot> cs = q->W.cs;
    cs.resize(cs.size() + 1);  // never an empty table
    if (!q->d_st.upload(L.st, "wide plan") || !q->d_cs.upload(cs, "wide plan") ||
        !q->d_vbox.upload(q->W.vbox, "wide plan") || !q->d_idxb.upload(hidx, "wide plan")) {
        delete q;
        return nullptr;
    }
    return q;
}

// out[8]: doubles per problem of BAbt, RSQrq, DCt, d (= lam = t), ux, pi, the work image; N
extern "C" int hpmpc_mi355x_wide_sizes(const hpmpc_mi355x_wide_plan* q, long long* out) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    const WLayout& L = q->W.L;
    const long long v[8] = {L.nB, L.nR, L.nG, L.nD, L.nU, L.nP, q->W.nIW, q->N};
    memcpy(out, v, sizeof v);
    return 0;
}

// out[6*(N+1)]: oB, oR, oG, oD, oU, oP of every stage (doubles inside one problem's arrays)
extern "C" int hpmpc_mi355x_wide_offsets(const hpmpc_mi355x_wide_plan* q, long long* out) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    for (int k = 0; k <= q->N; k++) {
        const WideStage& s = q->W.L.st[k];
        const long long v[6] = {s.oB, s.oR, s.oG, s.oD, s.oU, s.oP};
        memcpy(out + 6 * k, v, sizeof v);
    }
    return 0;
}

// d_ip2_res_mpc_hard_tv on problems [p0, p0 + count) of a device-resident batch (problem-major arrays with the
// per-problem sizes of hpmpc_mi355x_wide_sizes); kk / ret per problem, stat 5 * k_max per problem; `work` holds
// each problem's work image (the factor and iterate backup of its last iteration).  Asynchronous on `stream`.
extern "C" int hpmpc_mi355x_wide_ipm_batch(const hpmpc_mi355x_wide_plan* q, int nprob, int p0, int count,
                                           const double* BAbt, const double* RSQrq, const double* DCt, const double* d,
                                           double* ux, double* pi, double* lam, double* t, double* work, int k_max,
                                           double mu0, double mu_tol, double alpha_min, int warm_start,
                                           int compute_mult, int* kk, int* ret, double* stat, void* stream) {
    hk_set_error(0, nullptr);
    if (!q || nprob <= 0 || p0 < 0 || count < 0 || p0 + count > nprob || k_max < 0)
        return HPMPC_MI355X_EUNSUPPORTED;
    // every array the kernel dereferences unconditionally (DCt only when a stage has general constraints; stat is
    // nullable): a null one is a caller error, reported instead of faulting on the device
    if (!BAbt || !RSQrq || !d || !ux || !pi || !lam || !t || !work || !kk || !ret || (q->W.L.any_ng && !DCt)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_wide_ipm_batch: null array");
        return HPMPC_MI355X_EUNSUPPORTED;
    }
    WideIpmArgs a;
    ipm_args(q->W, nprob, p0, k_max, a);
    a.w.st = q->d_st.get();
    a.w.BAbt = BAbt;
    a.w.RSQ = RSQrq;
    a.w.DCt = DCt;
    a.w.idxb = q->d_idxb.get();
    a.mode = WI_IPM_RES;
    a.warm_start = warm_start;
    a.compute_mult = compute_mult;
    a.mu0 = mu0;
    a.mu_tol = mu_tol;
    a.alpha_min = alpha_min;
    a.cs = q->d_cs.get();
    a.vbox = q->d_vbox.get();
    a.d = d;
    a.ux = ux;
    a.pi = pi;
    a.lam = lam;
    a.t = t;
    a.iw = work;
    a.stat = stat;
    a.kk = kk;
    a.ret = ret;
    return count == 0 ? 0 : ipm_launch(q->W, a, count, (hipStream_t)stream);
}

// hpmpc_capi_dropin.cpp -- the reference-named single-problem entry points with hard constraints (drop-in for
// HPMPC's lqcp_solvers.h / mpc_solvers.h hot path): d_back_ric_rec_{sv,trf,trs}_tv_res, d_ip2_res_mpc_hard_tv and its
// single-Newton variant, d_ip2_mpc_hard_tv, the two KKT re-solves and the two residuals.  A problem beyond the
// 16-wide tile goes to the wide-stage path (hpmpc_capi_wide.cpp, hpmpc_capi_wide_ipm.cpp); every other call runs
// the tile kernels of hpmpc_kernels.hip.  There is no CPU fallback.
//
// Host marshalling:
//   * the caller's per-stage lib4 blocks (pointers may alias across stages) are copied stage by stage
//     into the pinned staging arena of the thread's device context, uploaded with one hipMemcpyAsync and solved
//     by a 1-problem launch;
//   * the reference's documented in-place side effects on hpRSQrq / hpBAbt (update_q / update_b
//     rows, box diagonal and gradient, d_back_ric_rec.c:197-209, :249-291) are applied to the caller's
//     buffers in the reference's stage order, and each stage's device copy receives exactly the
//     values the reference factorises for that stage;
//   * "memory" / "double_work_memory" hold this library's private device image (factor + persistent
//     IPM iterate) so that trs and d_kkt_solve_new_rhs_res_mpc_hard_tv can re-use it.
#include "hk_plan.h"
#include "hk_wide_args.h"

// Arena carve (doubles) for one problem.
Arena arena(const hpmpc_mi355x_plan* P, int k_max) {
    Arena A;
    size_t o = 0;
    auto take = [&](size_t n) {  // 128-B granules: every array starts on a cache line
        size_t r = o;
        o += (n + 15) / 16 * 16;
        return r;
    };
    const size_t n1 = P->N + 1;
    A.BAbt = take(P->packB);
    A.RSQ = take(P->packR);
    A.DCt = take(P->packG > 0 ? P->packG : 1);
    A.d = take(n1 * V32);
    A.ux = take(n1 * V16);
    A.pi = take(n1 * V16);
    A.lam = take(n1 * V32);
    A.t = take(n1 * V32);
    A.ws = take(ws_doubles(P->N));
    A.vb = take(n1 * V16);
    A.vq = take(n1 * V16);
    A.vQx = take(n1 * V16);
    A.vqx = take(n1 * V16);
    A.vPb = take(n1 * V16);
    A.stat = take(5 * (size_t)(k_max > 0 ? k_max : 1) + 8);
    A.ints = take(8);
    A.qctl = take(8);  // queue control of the one-entry queue the IPM entry points run (16 ints >= 6 + 3 slots)
    A.total = o;
    return A;
}

KArgs arena_args(const hpmpc_mi355x_plan* P, const Arena& A, double* dev) {
    KArgs a;
    (void)batch_args(a, P, nullptr, 1, 0, DCT_ARRAY, dev + A.DCt);  // the packed default layout: nothing to refuse
    a.BAbt = dev + A.BAbt;
    a.RSQ = dev + A.RSQ;
    a.d = dev + A.d;
    a.ux = dev + A.ux;
    a.pi = dev + A.pi;
    a.lam = dev + A.lam;
    a.t = dev + A.t;
    a.ws = dev + A.ws;
    a.vb = dev + A.vb;
    a.vq = dev + A.vq;
    a.vQx = dev + A.vQx;
    a.vqx = dev + A.vqx;
    a.vPb = dev + A.vPb;
    a.stat = dev + A.stat;
    a.kk = reinterpret_cast<int*>(dev + A.ints);
    a.ret = a.kk + 1;
    a.mu_out = dev + A.ints + 2;
    return a;
}

void stage_BAbt(const hpmpc_mi355x_plan* P, double* H, const Arena& A, double** hpBAbt) {
    for (int k = 0; k < P->N; k++) {
        const auto& s = P->st[k];
        const size_t n = (size_t)rup(s.nu + s.nx + 1, BS) * s.sdB;
        memcpy(H + A.BAbt + P->offB[k], hpBAbt[k], n * sizeof(double));
    }
}
void stage_RSQ(const hpmpc_mi355x_plan* P, double* H, const Arena& A, double** hpQ) {
    for (int k = 0; k <= P->N; k++) {
        const auto& s = P->st[k];
        const size_t n = (size_t)rup(s.nu + s.nx + 1, BS) * s.sdR;
        memcpy(H + A.RSQ + P->offR[k], hpQ[k], n * sizeof(double));
    }
}

// Per-stage length of a caller vector.  A length of 0 means the reference leaves that stage's buffer alone
// (pi / b / Pb at stage N, the constraint vectors of a stage without constraints), and so do vec_in / vec_out.
int vec_len(const hpmpc_mi355x_plan* P, VecKind kind, int k) {
    const auto& s = P->st[k];
    switch (kind) {
        case VEC_UX: return s.nu + s.nx;
        case VEC_PI: return s.nx1;
        default:  // constraint vectors: [lb (pnb) | ub (pnb) | lg (png) | ug (png)]
            return P->nb[k] + P->ng[k] > 0 ? 2 * s.pnb + 2 * rup(P->ng[k], BS) : 0;
    }
}
void vec_in(const hpmpc_mi355x_plan* P, VecKind kind, double* H, size_t off, double** v) {
    const int stride = kind == VEC_CV ? V32 : V16;
    for (int k = 0; k <= P->N; k++)
        if (const int n = vec_len(P, kind, k)) memcpy(H + off + k * stride, v[k], n * sizeof(double));
}
void vec_out(const hpmpc_mi355x_plan* P, VecKind kind, double** v, const double* H, size_t off) {
    const int stride = kind == VEC_CV ? V32 : V16;
    for (int k = 0; k <= P->N; k++)
        if (const int n = vec_len(P, kind, k)) memcpy(v[k], H + off + k * stride, n * sizeof(double));
}

bool run(int which, const KArgs& a, const char* name) {
    int e = launch(which, &a, 1, g_dev.stream);
    if (e) {
        char msg[128];
        snprintf(msg, sizeof msg, "%s launch failed (%d)", name, e);
        hk_set_error(HPMPC_MI355X_EHIP, msg);
        return false;
    }
    return true;
}

namespace {

// stages beyond the 16-wide tile (or its 32 constraint slots) run on the wide-stage path
bool wide_path(int N, const int* nx, const int* nu, const int* nb, int** idxb, const int* ng) {
    const char* why = nullptr;
    return !plan_supported(N, nx, nu, nb, idxb, ng, &why);
}

// What every tile-path entry point starts with: the error reset, the thread's plan for these sizes, its arena
// carve, and the device context sized for it (pinned arena cleared).  P is null when any of that failed.
struct Staged {
    hpmpc_mi355x_plan* P = nullptr;
    Arena A;
    double* H = nullptr;  // the pinned arena
    size_t bytes() const { return A.total * sizeof(double); }
    KArgs args() const { return arena_args(P, A, reinterpret_cast<double*>(g_dev.dev)); }
    // upload the carve, one launch, download and wait
    bool solve(int which, const KArgs& a, const char* name) const {
        return g_dev.up(bytes()) && run(which, a, name) && g_dev.down(bytes());
    }
    void in(VecKind kind, size_t off, double** v) const { vec_in(P, kind, H, off, v); }
    void out(VecKind kind, double** v, size_t off) const { vec_out(P, kind, v, H, off); }
};

Staged stage_begin(int N, const int* nx, const int* nu, const int* nb, int** idxb, const int* ng, int k_max) {
    Staged S;
    g_err = 0;
    hpmpc_mi355x_plan* P = thread_plan(N, nx, nu, nb, idxb, ng);
    if (!P) return S;
    S.A = arena(P, k_max);
    if (!g_dev.ensure(S.bytes())) return S;
    S.H = reinterpret_cast<double*>(g_dev.host);
    S.P = P;
    return S;
}

void stage_DCt(const Staged& S, double** hpDCt) {
    const hpmpc_mi355x_plan* P = S.P;
    for (int k = 0; k <= P->N; k++) {
        if (P->ng[k] == 0) continue;
        const auto& s = P->st[k];
        memcpy(S.H + S.A.DCt + P->offG[k], hpDCt[k],
               (size_t)rup(s.nu + s.nx, BS) * rup(P->ng[k], NCL) * sizeof(double));
    }
}
// Qx / qx of the general constraints ([box (pnb) | general (png)]): the box halves are applied on the
// host for sv / trf, so the device sees zeros there and only adds the general terms.
void stage_gen_q(const Staged& S, size_t off, double** v) {
    const hpmpc_mi355x_plan* P = S.P;
    for (int k = 0; k <= P->N; k++)
        for (int l = 0; l < P->ng[k]; l++) S.H[off + k * V16 + P->st[k].pnb + l] = v[k][P->st[k].pnb + l];
}

// sv / trf: stage copies receive exactly what the reference factorises for that stage; the caller's
// buffers get the reference's side effects, applied in its stage order (N .. 0).  trf has no q / qx / b.
void stage_ric_data(const Staged& S, const int* nb, int** idxb, int update_b, double** hpBAbt, double** b,
                    int update_q, double** hpQ, double** q, double** bd, double** Qx, double** qx) {
    const hpmpc_mi355x_plan* P = S.P;
    for (int k = P->N; k >= 0; k--) {
        const auto& s = P->st[k];
        const int nux = s.nu + s.nx, cnux = s.sdR;
        if (update_q)
            for (int j = 0; j < nux; j++) P4(hpQ[k], cnux, nux, j) = q[k][j];
        for (int l = 0; l < nb[k]; l++) {
            const int ii = idxb[k][l];
            P4(hpQ[k], cnux, ii, ii) = bd[k][l] + Qx[k][l];
        }
        if (qx)
            for (int l = 0; l < nb[k]; l++) P4(hpQ[k], cnux, nux, idxb[k][l]) += qx[k][l];
        memcpy(S.H + S.A.RSQ + P->offR[k], hpQ[k], (size_t)rup(nux + 1, BS) * cnux * sizeof(double));
        if (k < P->N) {
            if (update_b)
                for (int j = 0; j < s.nx1; j++) P4(hpBAbt[k], s.sdB, nux, j) = b[k][j];
            memcpy(S.H + S.A.BAbt + P->offB[k], hpBAbt[k], (size_t)rup(nux + 1, BS) * s.sdB * sizeof(double));
        }
    }
}

// sv / trs: the solution, and the multipliers / P b the caller asked for
void ric_out(const Staged& S, double** hux, int compute_pi, double** hpi, int compute_Pb, double** hPb) {
    S.out(VEC_UX, hux, S.A.ux);
    if (compute_pi) S.out(VEC_PI, hpi, S.A.pi);
    if (compute_Pb) S.out(VEC_PI, hPb, S.A.vPb);
}

// IPM / KKT re-solve: the iterate
void iterate_out(const Staged& S, double** ux, double** pi, double** lam, double** t) {
    S.out(VEC_UX, ux, S.A.ux);
    if (pi) S.out(VEC_PI, pi, S.A.pi);
    S.out(VEC_CV, lam, S.A.lam);
    S.out(VEC_CV, t, S.A.t);
}

}  // namespace

extern "C" int d_back_ric_rec_sv_tv_work_space_size_bytes(int N, int* nx, int* nu, int* nb, int* ng) {
    (void)N;
    (void)nx;
    (void)nu;
    (void)nb;
    (void)ng;
    return 64;  // all temporaries live on the device
}

extern "C" int d_back_ric_rec_sv_tv_memory_space_size_bytes(int N, int* nx, int* nu, int* nb, int* ng) {
    (void)nx;
    (void)nu;
    (void)nb;
    (void)ng;
    // the larger of the tile image and the wide-stage factor (nu+nx > 16 stages run on the wide path)
    const long long tile = (long long)(N + 1) * FSTRIDE * 8, wide = hk_wide_factor_bytes(N, nx, nu);
    return (int)(((tile > wide ? tile : wide) + 63) / 64 * 64);
}

extern "C" void d_back_ric_rec_sv_tv_res(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, int update_b,
                                         double** hpBAbt, double** b, int update_q, double** hpQ, double** q,
                                         double** bd, double** hpDCt, double** Qx, double** qx, double** hux,
                                         int compute_pi, double** hpi, int compute_Pb, double** hPb, double* memory,
                                         double* work) {
    (void)work;
    if (wide_path(N, nx, nu, nb, idxb, ng)) {
        hk_wide_sv_entry(N, nx, nu, nb, idxb, ng, update_b, hpBAbt, b, update_q, hpQ, q, bd, hpDCt, Qx, qx, hux,
                         compute_pi, hpi, compute_Pb, hPb, memory);
        return;
    }
    const Staged S = stage_begin(N, nx, nu, nb, idxb, ng, 1);
    if (!S.P) return;
    stage_ric_data(S, nb, idxb, update_b, hpBAbt, b, update_q, hpQ, q, bd, Qx, qx);
    KArgs a = S.args();
    a.compute_pi = compute_pi;
    a.compute_Pb = compute_Pb;
    if (S.P->ngt) {  // general constraints: DCt diag(Qx_g) DCt' and DCt qx_g on the device
        stage_DCt(S, hpDCt);
        stage_gen_q(S, S.A.vQx, Qx);
        stage_gen_q(S, S.A.vqx, qx);
        a.use_box = 1;
    }
    if (!S.solve(K_SV, a, "hk_ric_sv")) return;
    ric_out(S, hux, compute_pi, hpi, compute_Pb, hPb);
    memcpy(memory, S.H + S.A.ws, (size_t)(N + 1) * FSTRIDE * sizeof(double));
}

extern "C" void d_back_ric_rec_trf_tv_res(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                          double** hpQ, double** hpDCt, double** Qx, double** bd, double* memory,
                                          double* work) {
    (void)work;
    if (wide_path(N, nx, nu, nb, idxb, ng)) {
        hk_wide_trf_entry(N, nx, nu, nb, idxb, ng, hpBAbt, hpQ, hpDCt, Qx, bd, memory);
        return;
    }
    const Staged S = stage_begin(N, nx, nu, nb, idxb, ng, 1);
    if (!S.P) return;
    stage_ric_data(S, nb, idxb, 0, hpBAbt, nullptr, 0, hpQ, nullptr, bd, Qx, nullptr);
    KArgs a = S.args();
    if (S.P->ngt) {
        stage_DCt(S, hpDCt);
        stage_gen_q(S, S.A.vQx, Qx);
        a.use_box = 1;
    }
    if (!S.solve(K_TRF, a, "hk_ric_trf")) return;
    memcpy(memory, S.H + S.A.ws, (size_t)(N + 1) * FSTRIDE * sizeof(double));
}

extern "C" void d_back_ric_rec_trs_tv_res(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                          double** hb, double** hq, double** hpDCt, double** qx, double** hux,
                                          int compute_pi, double** hpi, int compute_Pb, double** hPb, double* memory,
                                          double* work) {
    (void)work;
    if (wide_path(N, nx, nu, nb, idxb, ng)) {
        hk_wide_trs_entry(N, nx, nu, nb, idxb, ng, hpBAbt, hb, hq, hpDCt, qx, hux, compute_pi, hpi, compute_Pb,
                          hPb, memory);
        return;
    }
    const Staged S = stage_begin(N, nx, nu, nb, idxb, ng, 1);
    if (!S.P) return;
    stage_BAbt(S.P, S.H, S.A, hpBAbt);
    memcpy(S.H + S.A.ws, memory, (size_t)(N + 1) * FSTRIDE * sizeof(double));
    S.in(VEC_UX, S.A.vq, hq);
    S.in(VEC_PI, S.A.vb, hb);
    if (!compute_Pb) S.in(VEC_PI, S.A.vPb, hPb);
    for (int k = 0; k <= N; k++)
        if (nb[k] > 0) memcpy(S.H + S.A.vqx + k * V16, qx[k], nb[k] * sizeof(double));
    if (S.P->ngt) {
        stage_DCt(S, hpDCt);
        stage_gen_q(S, S.A.vqx, qx);
    }
    KArgs a = S.args();
    a.use_box = 1;
    a.compute_pi = compute_pi;
    a.compute_Pb = compute_Pb;
    if (!S.solve(K_TRS, a, "hk_ric_trs")) return;
    ric_out(S, hux, compute_pi, hpi, compute_Pb, hPb);
}

extern "C" int d_ip2_res_mpc_hard_tv_work_space_size_bytes(int N, int* nx, int* nu, int* nb, int* ng) {
    // the larger of the tile path's image and the wide-stage IPM's (problems beyond the tile run there)
    std::vector<int> nuN(nu, nu + N + 1);
    nuN[N] = 0;
    const long long tile = ws_doubles(N) * 8, wide = hk_wide_ipm_bytes(N, nx, nuN.data(), nb, ng);
    return (int)(((tile > wide ? tile : wide) + 63) / 64 * 64);
}

namespace {

// Shared body of d_ip2_res_mpc_hard_tv and its single-Newton variant.  For the variant, ux0/pi0/lam0/t0
// hold the start iterate (lam0/t0 as [lower(nb) | upper(nb)], d_aux_ip_hard_lib4.c:153-213).
int ipm_entry(int single_newton, int phase1_only, int* kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
              double* stat, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng, double** pBAbt, double** pQ,
              double** pDCt, double** d, double** ux, int compute_mult, double** pi, double** lam, double** t,
              double* double_work_memory, double** ux0, double** pi0, double** lam0, double** t0) {
    if (wide_path(N, nx, nu_N, nb, idxb, ng))
        return hk_wide_ipm_entry(single_newton ? WI_NEWTON : phase1_only ? WI_IPM_P1 : WI_IPM_RES, kk, k_max, mu0,
                                 mu_tol, alpha_min, warm_start, stat, N, nx, nu_N, nb, idxb, ng, pBAbt, pQ, pDCt, d, ux,
                                 compute_mult, pi, lam, t, double_work_memory, ux0, pi0, lam0, t0);
    const Staged S = stage_begin(N, nx, nu_N, nb, idxb, ng, k_max);
    if (!S.P) return g_err;
    const hpmpc_mi355x_plan* P = S.P;
    if (single_newton && P->ngt) {  // the reference stops here too (d_aux_ip_hard_lib4.c:197-208)
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "single Newton step with general constraints");
        return g_err;
    }
    double* H = S.H;
    const Arena& A = S.A;
    stage_BAbt(P, H, A, pBAbt);
    stage_RSQ(P, H, A, pQ);
    S.in(VEC_CV, A.d, d);
    stage_DCt(S, pDCt);
    if (single_newton) {
        S.in(VEC_UX, A.ux, ux0);
        S.in(VEC_PI, A.pi, pi0);
        for (int k = 0; k <= N; k++) {
            const int pnb = P->st[k].pnb;
            for (int l = 0; l < nb[k]; l++) {
                H[A.lam + k * V32 + l] = lam0[k][l];
                H[A.lam + k * V32 + pnb + l] = lam0[k][nb[k] + l];
                H[A.t + k * V32 + l] = t0[k][l];
                H[A.t + k * V32 + pnb + l] = t0[k][nb[k] + l];
            }
        }
    } else if (warm_start) {
        S.in(VEC_UX, A.ux, ux);
    }
    KArgs a = S.args();
    a.k_max = k_max;
    a.mu0 = mu0;
    a.mu_tol = mu_tol;
    a.alpha_min = alpha_min;
    a.warm_start = warm_start;
    a.compute_mult = compute_mult;
    a.single_newton = single_newton;
    a.phase1_only = phase1_only;
    // the whole solve in one launch (hk_ipm_solo): one workgroup runs init and every iteration's passes back to
    // back, its stage data and factor records resident in one XCD's L2
    if (!g_dev.up(S.bytes())) return g_err;
    if (hk_launch(K_SOLO, &a, 1, g_dev.stream)) {
        hk_set_error(HPMPC_MI355X_EHIP, "hk_ipm_solo launch failed");
        return g_err;
    }
    if (!g_dev.down(S.bytes())) return g_err;
    const int* iv = reinterpret_cast<const int*>(H + A.ints);
    *kk = iv[0];
    if (iv[1] == HPMPC_MI355X_EMW) {
        // the multi-wave kernel abandoned the solve (an expired hand-over wait: a bug, never a data condition); its
        // stat holds diagnostics and its iterate is not a solution, so nothing is copied out
        hk_set_error(HPMPC_MI355X_EMW, "hk_ipm_solo_mw: expired hand-over wait, solve abandoned");
        return g_err;
    }
    for (int i = 0; i < 5 * iv[0]; i++) stat[i] = H[A.stat + i];
    // d_ip2_mpc_hard_tv without constraints solves into its workspace only (d_ip2_hard.c:282-291)
    if (!(phase1_only && P->nbt == 0)) iterate_out(S, ux, pi, lam, t);
    memcpy(double_work_memory, H + A.ws, ws_doubles(N) * sizeof(double));
    return iv[1];
}

// Shared body of the two KKT re-solves.  p1 (d_kkt_solve_new_rhs_mpc_hard_tv): the factor of the IPM's last
// iteration is in the workspace, so pQ is not read; ux is an input too; pi is written only with compute_mult; the
// workspace goes back to the caller (left as the IPM wrote it, apart from qx and Pb, as the reference).
void kkt_entry(int p1, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng, double** pBAbt, double** b,
               double** pQ, double** q, double** pDCt, double** d, double** ux, int compute_mult, double** pi,
               double** lam, double** t, double* double_work_memory) {
    if (wide_path(N, nx, nu_N, nb, idxb, ng)) {
        hk_wide_kkt_entry(p1, N, nx, nu_N, nb, idxb, ng, pBAbt, b, pQ, q, pDCt, d, ux, compute_mult, pi, lam, t,
                          double_work_memory);
        return;
    }
    const Staged S = stage_begin(N, nx, nu_N, nb, idxb, ng, 1);
    if (!S.P) return;
    stage_BAbt(S.P, S.H, S.A, pBAbt);
    if (!p1) stage_RSQ(S.P, S.H, S.A, pQ);
    S.in(VEC_CV, S.A.d, d);
    stage_DCt(S, pDCt);
    memcpy(S.H + S.A.ws, double_work_memory, ws_doubles(N) * sizeof(double));
    S.in(VEC_UX, S.A.vq, q);
    if (p1) S.in(VEC_UX, S.A.ux, ux);
    S.in(VEC_PI, S.A.vb, b);
    KArgs a = S.args();
    a.compute_mult = compute_mult;
    if (!S.solve(p1 ? K_KKT_P1 : K_KKT, a, p1 ? "hk_kkt_new_rhs_p1" : "hk_kkt_new_rhs")) return;
    iterate_out(S, ux, !p1 || compute_mult ? pi : nullptr, lam, t);
    if (p1) memcpy(double_work_memory, S.H + S.A.ws, ws_doubles(N) * sizeof(double));
}

// Shared body of the two residuals.  plain (d_res_mpc_hard_tv): the sign convention of mpc_solvers/d_res_ip_hard.c
// and no r_m; otherwise mu is an input as well, left untouched when there are no constraints
// (d_res_ip_res_hard.c:309-313).
void res_entry(int plain, int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt, double** hb,
               double** hpQ, double** hq, double** hux, double** hpDCt, double** hd, double** hpi, double** hlam,
               double** ht, double** hrq, double** hrb, double** hrd, double** hrm, double* mu) {
    if (wide_path(N, nx, nu, nb, idxb, ng)) {
        hk_wide_res_entry(plain, N, nx, nu, nb, idxb, ng, hpBAbt, hb, hpQ, hq, hux, hpDCt, hd, hpi, hlam, ht, hrq, hrb,
                          hrd, hrm, mu);
        return;
    }
    const Staged S = stage_begin(N, nx, nu, nb, idxb, ng, 1);
    if (!S.P) return;
    const Arena& A = S.A;
    stage_BAbt(S.P, S.H, A, hpBAbt);
    stage_RSQ(S.P, S.H, A, hpQ);
    S.in(VEC_CV, A.d, hd);
    stage_DCt(S, hpDCt);
    S.in(VEC_UX, A.vq, hq);
    S.in(VEC_UX, A.ux, hux);
    S.in(VEC_PI, A.vb, hb);
    S.in(VEC_PI, A.pi, hpi);
    S.in(VEC_CV, A.lam, hlam);
    S.in(VEC_CV, A.t, ht);
    KArgs a = S.args();
    if (plain)
        a.res_plain = 1;
    else
        S.H[A.ints + 2] = *mu;
    if (!S.solve(K_RES, a, "hk_res")) return;
    const size_t n1 = N + 1, rq = A.ws, rb = rq + n1 * V16, rd = rb + n1 * V16, rm = rd + n1 * V32;
    S.out(VEC_UX, hrq, rq);
    S.out(VEC_PI, hrb, rb);
    S.out(VEC_CV, hrd, rd);
    if (!plain) S.out(VEC_CV, hrm, rm);
    *mu = S.H[A.ints + 2];
}

}  // namespace

extern "C" int d_ip2_res_mpc_hard_tv(int* kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                                     double* stat, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng,
                                     double** pBAbt, double** pQ, double** pDCt, double** d, double** ux,
                                     int compute_mult, double** pi, double** lam, double** t,
                                     double* double_work_memory) {
    return ipm_entry(0, 0, kk, k_max, mu0, mu_tol, alpha_min, warm_start, stat, N, nx, nu_N, nb, idxb, ng, pBAbt, pQ,
                     pDCt, d, ux, compute_mult, pi, lam, t, double_work_memory, nullptr, nullptr, nullptr, nullptr);
}

extern "C" int d_ip2_res_mpc_hard_tv_single_newton_step(int* kk, int k_max, double mu0, double mu_tol,
                                                        double alpha_min, int warm_start, double* stat, int N,
                                                        int* nx, int* nu_N, int* nb, int** idxb, int* ng,
                                                        double** pBAbt, double** pQ, double** pDCt, double** d,
                                                        double** ux, int compute_mult, double** pi, double** lam,
                                                        double** t, double* double_work_memory, double** ux0,
                                                        double** pi0, double** lam0, double** t0) {
    return ipm_entry(1, 0, kk, k_max, mu0, mu_tol, alpha_min, warm_start, stat, N, nx, nu_N, nb, idxb, ng, pBAbt, pQ,
                     pDCt, d, ux, compute_mult, pi, lam, t, double_work_memory, ux0, pi0, lam0, t0);
}

extern "C" void d_kkt_solve_new_rhs_res_mpc_hard_tv(int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng,
                                                    double** pBAbt, double** b, double** pQ, double** q,
                                                    double** pDCt, double** d, double** ux, int compute_mult,
                                                    double** pi, double** lam, double** t,
                                                    double* double_work_memory) {
    kkt_entry(0, N, nx, nu_N, nb, idxb, ng, pBAbt, b, pQ, q, pDCt, d, ux, compute_mult, pi, lam, t,
              double_work_memory);
}

extern "C" void d_res_res_mpc_hard_tv(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                      double** hb, double** hpQ, double** hq, double** hux, double** hpDCt,
                                      double** hd, double** hpi, double** hlam, double** ht, double* work,
                                      double** hrq, double** hrb, double** hrd, double** hrm, double* mu) {
    (void)work;
    res_entry(0, N, nx, nu, nb, idxb, ng, hpBAbt, hb, hpQ, hq, hux, hpDCt, hd, hpi, hlam, ht, hrq, hrb, hrd, hrm, mu);
}

// ------------------------------------------------------------------------------------------------
// The alternate IPM of mpc_solvers/d_ip2_hard.c (phase-1 Mehrotra loop alone), its KKT re-solve and the
// plain residuals of mpc_solvers/d_res_ip_hard.c, on the same kernels (KArgs.phase1_only / res_plain).
// ------------------------------------------------------------------------------------------------
extern "C" int d_ip2_mpc_hard_tv_work_space_size_bytes(int N, int* nx, int* nu, int* nb, int* ng) {
    return d_ip2_res_mpc_hard_tv_work_space_size_bytes(N, nx, nu, nb, ng);
}

extern "C" int d_ip2_mpc_hard_tv(int* kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                                 double* stat, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng,
                                 double** pBAbt, double** pQ, double** pDCt, double** d, double** ux,
                                 int compute_mult, double** pi, double** lam, double** t,
                                 double* double_work_memory) {
    return ipm_entry(0, 1, kk, k_max, mu0, mu_tol, alpha_min, warm_start, stat, N, nx, nu_N, nb, idxb, ng, pBAbt,
                     pQ, pDCt, d, ux, compute_mult, pi, lam, t, double_work_memory, nullptr, nullptr, nullptr,
                     nullptr);
}

extern "C" void d_kkt_solve_new_rhs_mpc_hard_tv(int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng,
                                                double** pBAbt, double** r_A, double** pQ, double** r_H,
                                                double** pDCt, double** r_C, double** ux, int compute_mult,
                                                double** pi, double** lam, double** t, double* double_work_memory) {
    kkt_entry(1, N, nx, nu_N, nb, idxb, ng, pBAbt, r_A, pQ, r_H, pDCt, r_C, ux, compute_mult, pi, lam, t,
              double_work_memory);
}

extern "C" void d_res_mpc_hard_tv(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                  double** hb, double** hpQ, double** hq, double** hux, double** hpDCt, double** hd,
                                  double** hpi, double** hlam, double** ht, double** hrq, double** hrb, double** hrd,
                                  double* mu) {
    res_entry(1, N, nx, nu, nb, idxb, ng, hpBAbt, hb, hpQ, hq, hux, hpDCt, hd, hpi, hlam, ht, hrq, hrb, hrd, nullptr,
              mu);
}

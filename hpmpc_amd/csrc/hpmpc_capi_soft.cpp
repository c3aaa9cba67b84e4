// hpmpc_capi_soft.cpp -- the reference-named soft-constraint entry points: d_ip2_mpc_soft_tv, d_res_mpc_soft_tv
// and their size queries, on the passes of hk_soft.hip and the tile Riccati kernels.
#include <algorithm>

#include "hk_plan.h"

// ================================================================================================
// Soft-constraint IPM d_ip2_mpc_soft_tv (mpc_solvers/d_ip2_soft.c:42-547, include/mpc_solvers.h:69-70):
// the constraint passes of hk_soft.hip around the tile Riccati kernels, one host round trip (the exit
// flag) per iteration.  Limits (HPMPC_MI355X_EUNSUPPORTED, DESIGN.md soft constraints): ng = 0, nu[N] = 0,
// round_up(nb + ns, 4) <= 16 per stage, b_k read inside BAbt_k with the reference's stride
// (d_ip2_soft.c:172), and no soft-gradient write of the reference into a Zl its pass still reads.
// ================================================================================================
const char* soft_unsupported(int N, const int* nx, const int* nu, const int* ng) {
    if (N < 1 || nu[N] != 0) return "soft IPM: N >= 1 and nu[N] = 0 required";
    for (int k = 0; k <= N; k++)
        if (ng[k] != 0) return "soft IPM with general constraints (ng > 0)";
    for (int k = 0; k < N; k++) {
        const int nux = nu[k] + nx[k], nx1 = nx[k + 1];
        const long idx = (long)(nux / BS) * BS * rup(nx1, BS) + nux % BS + BS * (long)(nx1 > 0 ? nx1 - 1 : 0);
        if (nx1 > 0 && idx >= (long)rup(nux + 1, BS) * rup(nx1, NCL))
            return "soft IPM: the reference reads b_k outside BAbt_k here (stride round_up(nx,4), d_ip2_soft.c:172)";
    }
    return nullptr;
}

// soft layout (doubles): per-stage constraint vectors, then the flat Qx / qx | Zl / zl block in the reference's
// carve order with its padding (d_ip2_soft.c:244-260)
const char* soft_layout(int N, const int* nx, const int* nu, const int* nb, const int* ns, SoftLayout& L) {
    std::vector<SoftStage>& ss = L.st;
    ss.assign(N + 1, SoftStage());
    long sC = 0, sD = 0, sZ = 0, F = 0;
    int padM = 0;
    for (int k = 0; k <= N; k++) {
        SoftStage& s = ss[k];
        memset(&s, 0, sizeof s);
        s.nu = k < N ? nu[k] : 0;
        s.nx = nx[k];
        s.nx1 = k < N ? nx[k + 1] : 0;
        s.nb = nb[k];
        s.ns = ns[k];
        s.pnb = rup(nb[k], BS);
        s.pns = rup(ns[k], BS);
        s.oC = (int)sC;
        sC += 2 * s.pnb + 4 * s.pns;
        s.oD = (int)sD;
        sD += 2 * s.pnb + 2 * s.pns;
        s.oZ = (int)sZ;
        sZ += 2 * s.pns;
        s.oQ = (int)F;
        F += 2 * (s.pnb + s.pns);
        padM = std::max(padM, 2 * (s.pnb + s.pns));
    }
    for (int k = 0; k <= N; k++) {
        ss[k].oZl = (int)F;
        F += 4 * ss[k].pns;
    }
    L.sC = sC;
    L.sD = sD;
    L.sZ = sZ;
    L.sF = F + padM + 16;
    for (int k = 0; k <= N; k++) {  // where the soft gradient term goes (d_aux_ip_soft_lib4.c:557, :601)
        SoftStage& s = ss[k];
        const int pnbs = rup(s.nb + s.ns, BS);
        s.oS = s.oQ + s.pnb + s.pns + (s.nb > 0 ? pnbs + s.nb : s.nb);
        for (int i = 0; s.nb > 0 && i < s.ns; i++)
            for (int j = k; j <= N; j++)
                if (s.oS + i >= ss[j].oZl && s.oS + i < ss[j].oZl + 2 * ss[j].pns)
                    return "soft IPM: the reference's soft-gradient write lands in a Zl read later in the same pass";
    }
    return nullptr;
}

double soft_mu_scal(int N, const int* nb, const int* ns) {
    double m = 0.0;
    for (int k = 0; k <= N; k++) m += 2 * nb[k] + 4 * ns[k];
    return m > 0.0 ? 1.0 / m : 0.0;
}

void soft_ric_flags(KArgs& a, int compute_mult) {
    a.use_box = 1;
    a.update_q = 1;
    a.update_b = 0;
    a.compute_pi = compute_mult;
    a.compute_Pb = 1;
}

SoftArgs soft_scalars(int N, int nprob, int p0, int k_max, int warm_start, double mu0, double mu_tol, double alpha_min,
                      double mu_scal) {
    SoftArgs s;
    memset(&s, 0, sizeof s);
    s.N = N;
    s.nprob = nprob;
    s.p0 = p0;
    s.k_max = k_max;
    s.warm_start = warm_start;
    s.nq = (N + 4) / 4;
    s.mu0 = mu0;
    s.mu_tol = mu_tol;
    s.alpha_min = alpha_min;
    s.mu_scal = mu_scal;
    return s;
}

namespace {

bool soft_launch(int which, const SoftArgs& s) {
    if (hk_soft_launch(which, &s, 1, g_dev.stream)) {
        hk_set_error(HPMPC_MI355X_EHIP, "hk_soft_pass launch failed");
        return false;
    }
    return true;
}

}  // namespace

extern "C" int d_ip2_mpc_soft_tv_work_space_size_bytes(int N, int* nx, int* nu, int* nb, int* ng, int* ns) {
    (void)N;
    (void)nx;
    (void)nu;
    (void)nb;
    (void)ng;
    (void)ns;
    return 64;  // iterate, factor and work vectors live on the device
}

extern "C" int d_ip2_mpc_soft_tv(int* kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                                 double* stat, int N, int* nx, int* nu, int* nb, int** idxb, int* ng, int* ns,
                                 double** pBAbt, double** pQ, double** Z, double** z, double** pDCt, double** d,
                                 double** ux, int compute_mult, double** pi, double** lam, double** t,
                                 double* double_work_memory) {
    (void)pDCt;
    (void)double_work_memory;
    g_err = 0;
    if (const char* why = soft_unsupported(N, nx, nu, ng)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, why);
        return g_err;
    }
    const double mu_scal = soft_mu_scal(N, nb, ns);  // every ng is 0 here
    if (mu_scal == 0.0) {  // the reference solves into its workspace and leaves every output untouched (:273-284)
        *kk = 0;
        return 0;
    }
    std::vector<int> nbs(N + 1);
    for (int k = 0; k <= N; k++) nbs[k] = nb[k] + ns[k];
    hpmpc_mi355x_plan* P = thread_plan(N, nx, nu, nbs.data(), idxb, ng);
    if (!P) return g_err;
    SoftLayout SL;
    if (const char* why = soft_layout(N, nx, nu, nb, ns, SL)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, why);
        return g_err;
    }
    const std::vector<SoftStage>& ss = SL.st;
    const long sC = SL.sC, sD = SL.sD, sZ = SL.sZ, sF = SL.sF;
    Arena A = arena(P, 1);
    const size_t n1 = N + 1, v16 = n1 * V16;
    size_t o = A.total;
    auto take = [&](size_t n) {
        size_t r = o;
        o += (n + 7) / 8 * 8;
        return r;
    };
    const size_t oScal = take(4), oIst = take(4), oStat = take(5 * (size_t)(k_max > 0 ? k_max : 1) + 8),
                 oTab = take((sizeof(SoftStage) * n1 + 7) / 8), oIdx = take((n1 * 16 * sizeof(int) + 7) / 8),
                 oD = take(sD + 1), oZ = take(sZ + 1), oz = take(sZ + 1), oF = take(sF), oUx = take(v16),
                 oPi = take(v16);
    size_t oCv[6];
    for (int i = 0; i < 6; i++) oCv[i] = take(sC + 1);
    const size_t total = o;
    if (!g_dev.ensure(total * sizeof(double))) return g_err;
    double* H = reinterpret_cast<double*>(g_dev.host);
    stage_BAbt(P, H, A, pBAbt);
    stage_RSQ(P, H, A, pQ);
    memcpy(H + oTab, ss.data(), sizeof(SoftStage) * n1);
    idxb_table(N, nbs.data(), idxb, reinterpret_cast<int*>(H + oIdx));  // the pinned arena is cleared (ensure)
    for (int k = 0; k <= N; k++) {
        const SoftStage& s = ss[k];
        const int nux = s.nu + s.nx;
        for (int l = 0; l < nux; l++) H[A.vq + k * V16 + l] = P4(pQ[k], rup(nux, NCL), nux, l);
        if (k < N) {  // b_k with the reference's stride round_up(nx_{k+1}, 4) (d_ip2_soft.c:172)
            const double* row = pBAbt[k] + (nux / BS) * BS * rup(s.nx1, BS) + nux % BS;
            for (int j = 0; j < s.nx1; j++) H[A.vb + k * V16 + j] = row[BS * j];
        }
        memcpy(H + oD + s.oD, d[k], (2 * s.pnb + 2 * s.pns) * sizeof(double));
        if (s.ns > 0) {
            memcpy(H + oZ + s.oZ, Z[k], 2 * s.pns * sizeof(double));
            memcpy(H + oz + s.oZ, z[k], 2 * s.pns * sizeof(double));
        }
        if (warm_start) memcpy(H + oUx + k * V16, ux[k], nux * sizeof(double));
    }
    double* D = reinterpret_cast<double*>(g_dev.dev);
    KArgs a = arena_args(P, A, D);
    soft_ric_flags(a, compute_mult);
    KArgs a2 = a;
    a2.compute_Pb = 0;
    SoftArgs s = soft_scalars(N, 1, 0, k_max, warm_start, mu0, mu_tol, alpha_min, mu_scal);
    s.st =reinterpret_cast<const SoftStage*>(D + oTab);
    s.idxb = reinterpret_cast<const int*>(D + oIdx);
    s.d = D + oD;
    s.Z = D + oZ;
    s.z = D + oz;
    s.t = D + oCv[0];
    s.lam = D + oCv[1];
    s.dt = D + oCv[2];
    s.dlam = D + oCv[3];
    s.lamt = D + oCv[4];
    s.tinv = D + oCv[5];
    s.flat = D + oF;
    s.ux = D + oUx;
    s.pi = D + oPi;
    s.dux = D + A.ux;
    s.dpi = D + A.pi;
    s.vQx = D + A.vQx;
    s.vqx = D + A.vqx;
    s.scal = D + oScal;
    s.ist = reinterpret_cast<int*>(D + oIst);
    s.stat = D + oStat;
    if (!g_dev.up(total * sizeof(double)) || !soft_launch(SOFT_INIT, s)) return g_err;
    const int* hist = reinterpret_cast<const int*>(H + oIst);
    for (int it = 0; it < k_max; it++) {
        if (!soft_launch(SOFT_HESS, s) || !run(K_SV, a, "hk_ric_sv") || !soft_launch(SOFT_PRED, s) ||
            !run(K_TRS, a2, "hk_ric_trs") || !soft_launch(SOFT_CORR, s))
            return g_err;
        if (!hip_ok(hipMemcpyAsync(H + oIst, D + oIst, 4 * sizeof(int), hipMemcpyDeviceToHost, g_dev.stream),
                    "D2H") ||
            !hip_ok(hipStreamSynchronize(g_dev.stream), "sync"))
            return g_err;
        if (!hist[1]) break;
    }
    if (!g_dev.down(total * sizeof(double))) return g_err;
    *kk = hist[0];
    for (int i = 0; i < 5 * hist[0]; i++) stat[i] = H[oStat + i];
    vec_out(P, VEC_UX, ux, H, oUx);
    vec_out(P, VEC_PI, pi, H, oPi);
    for (int k = 0; k <= N; k++) {
        const SoftStage& st = ss[k];
        const int nc = 2 * st.pnb + 4 * st.pns;
        if (nc > 0) {
            memcpy(lam[k], H + oCv[1] + st.oC, nc * sizeof(double));
            memcpy(t[k], H + oCv[0] + st.oC, nc * sizeof(double));
        }
    }
    return hist[2];
}

// ------------------------------------------------------------------------------------------------
// d_res_mpc_soft_tv (mpc_solvers/d_res_ip_soft.c:38-268, include/mpc_solvers.h:71): hk_soft_res on a copy of
// every array of the call.  The output vectors are uploaded first, so the entries the reference does not write
// (padding, and stage N's input rows of r_q, :199-200) come back as the caller left them.  General constraints
// are supported (the residual has no soft-gradient quirk); stage 0's pi_{-1} (nx_0 > 0) reads as zero.
// ------------------------------------------------------------------------------------------------
extern "C" void d_res_mpc_soft_tv(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, int* ns, double** hpBAbt,
                                  double** hpQ, double** hq, double** hZ, double** hz, double** hux, double** hpDCt,
                                  double** hd, double** hpi, double** hlam, double** ht, double** hrq, double** hrb,
                                  double** hrd, double** hrz, double* mu) {
    g_err = 0;
    if (N < 0) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "d_res_mpc_soft_tv: N < 0");
        return;
    }
    std::vector<SoftResStage> st(N + 1);
    std::vector<int> ints;
    size_t o = 0;
    auto take = [&](size_t n) {
        size_t r = o;
        o += (n + 7) / 8 * 8;
        return (int)r;
    };
    for (int k = 0; k <= N; k++) {
        SoftResStage& s = st[k];
        s.nu = nu[k];
        s.nx = nx[k];
        s.nb = nb[k];
        s.ng = ng[k];
        s.ns = ns[k];
        s.nx1 = k < N ? nx[k + 1] : 0;
        s.nu1 = k < N ? nu[k + 1] : 0;
        s.pnb = rup(nb[k], BS);
        s.png = rup(ng[k], BS);
        s.pns = rup(ns[k], BS);
        const int nux = s.nu + s.nx, ncv = 2 * s.pnb + 2 * s.png + 4 * s.pns, nrd = 2 * s.pnb + 2 * s.png + 2 * s.pns;
        s.sdB = rup(s.nx1, NCL);
        s.sdQ = rup(nux, NCL);
        s.sdG = rup(ng[k], NCL);
        s.oB = k < N ? take((size_t)rup(nux + 1, BS) * s.sdB) : -1;
        s.oQ = take((size_t)rup(nux + 1, BS) * s.sdQ);
        s.oq = take(nux);
        s.oZ = take(2 * s.pns);
        s.oz = take(2 * s.pns);
        s.oux = take(nux);
        s.oG = ng[k] > 0 ? take((size_t)rup(nux, BS) * s.sdG) : -1;
        s.od = take(nrd);
        s.opi = k < N ? take(s.nx1) : -1;
        s.olam = take(ncv);
        s.ot = take(ncv);
        s.orq = take(nux);
        s.orb = k < N ? take(s.nx1) : -1;
        s.ord = take(nrd);
        s.orz = take(2 * s.pns);
        s.oI = (int)ints.size();
        // the soft constraints read idxb[k][nu_k + i] (:107), so the row is copied that far
        const int nI = std::max(nb[k], ns[k] > 0 ? nu[k] + ns[k] : 0);
        for (int j = 0; j < nI; j++) ints.push_back(idxb[k][j]);
    }
    for (int k = 0; k <= N; k++) {
        st[k].oux1 = k < N ? st[k + 1].oux : -1;
        st[k].opim1 = k > 0 ? st[k - 1].opi : -1;
    }
    const int omu = take(1);
    const size_t oSt = take((sizeof(SoftResStage) * (N + 1) + 7) / 8), oIdx = take((4 * ints.size() + 7) / 8 + 1);
    const size_t bytes = o * sizeof(double);
    if (!g_dev.ensure(bytes)) return;
    double* H = reinterpret_cast<double*>(g_dev.host);
    double* D = reinterpret_cast<double*>(g_dev.dev);
    auto cp = [&](int off, const double* src, size_t n) {
        if (off >= 0 && n > 0) memcpy(H + off, src, n * sizeof(double));
    };
    for (int k = 0; k <= N; k++) {
        const SoftResStage& s = st[k];
        const int nux = s.nu + s.nx, ncv = 2 * s.pnb + 2 * s.png + 4 * s.pns, nrd = 2 * s.pnb + 2 * s.png + 2 * s.pns;
        if (k < N) cp(s.oB, hpBAbt[k], (size_t)rup(nux + 1, BS) * s.sdB);
        cp(s.oQ, hpQ[k], (size_t)rup(nux + 1, BS) * s.sdQ);
        cp(s.oq, hq[k], nux);
        if (ns[k] > 0) {
            cp(s.oZ, hZ[k], 2 * s.pns);
            cp(s.oz, hz[k], 2 * s.pns);
            cp(s.orz, hrz[k], 2 * s.pns);
        }
        cp(s.oux, hux[k], nux);
        if (ng[k] > 0) cp(s.oG, hpDCt[k], (size_t)rup(nux, BS) * s.sdG);
        if (nrd > 0) {
            cp(s.od, hd[k], nrd);
            cp(s.ord, hrd[k], nrd);
            cp(s.olam, hlam[k], ncv);
            cp(s.ot, ht[k], ncv);
        }
        if (k < N) {
            cp(s.opi, hpi[k], s.nx1);
            cp(s.orb, hrb[k], s.nx1);
        }
        cp(s.orq, hrq[k], nux);
    }
    memcpy(H + oSt, st.data(), sizeof(SoftResStage) * (N + 1));
    if (!ints.empty()) memcpy(H + oIdx, ints.data(), 4 * ints.size());
    SoftResArgs a;
    a.N = N;
    a.st = reinterpret_cast<const SoftResStage*>(D + oSt);
    a.idxb = reinterpret_cast<const int*>(D + oIdx);
    a.buf = D;
    a.omu = omu;
    if (!g_dev.up(bytes)) return;
    if (hk_soft_res_launch(&a, g_dev.stream)) {
        hk_set_error(HPMPC_MI355X_EHIP, "hk_soft_res launch failed");
        return;
    }
    if (!g_dev.down(bytes)) return;
    for (int k = 0; k <= N; k++) {
        const SoftResStage& s = st[k];
        const int nux = s.nu + s.nx, nrd = 2 * s.pnb + 2 * s.png + 2 * s.pns;
        memcpy(hrq[k], H + s.orq, nux * sizeof(double));
        if (k < N && s.nx1 > 0) memcpy(hrb[k], H + s.orb, s.nx1 * sizeof(double));
        if (nrd > 0) memcpy(hrd[k], H + s.ord, nrd * sizeof(double));
        if (ns[k] > 0) memcpy(hrz[k], H + s.orz, 2 * s.pns * sizeof(double));
    }
    *mu = H[omu];
}

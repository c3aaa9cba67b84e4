// hpmpc_capi_soft_batch.cpp -- the batched, device-resident soft-constraint IPM: hpmpc_mi355x_soft_plan_* and
// hpmpc_mi355x_ipm_soft_batch, d_ip2_mpc_soft_tv (mpc_solvers/d_ip2_soft.c:83-547) on problems whose arrays are
// already in HBM, every iteration of every problem in one launch of hk_soft_ipm (hk_soft_ipm.hip).
//
// A soft plan wraps a tile plan on nb + ns boxes per stage (the plan the reference-named entry point solves on) and
// the soft layout; what it refuses, it refuses through the functions that entry point calls (soft_unsupported,
// soft_layout, plan_supported).  Per problem the caller passes d, Z / z, lam / t in the reference's per-stage
// layouts at the offsets of hpmpc_mi355x_soft_offsets, ux / pi with 16 doubles per stage, and a workspace:
//   [ factor (N+1) FSTRIDE | dux dpi b q Qx qx Pb, (N+1) 16 each | dt dlam lamt tinv | flat Qx qx Zl zl | scal | ist ]
// (the flat block in the reference's carve order with its padding, hk_soft_args.h).
#include "hk_soft_plan.h"

extern "C" void hpmpc_mi355x_soft_plan_destroy(hpmpc_mi355x_soft_plan* S) { delete S; }

extern "C" hpmpc_mi355x_soft_plan* hpmpc_mi355x_soft_plan_create(int N, const int* nx, const int* nu, const int* nb,
                                                                 const int* const* idxb, const int* ng,
                                                                 const int* ns) {
    g_err = 0;
    if (const char* why = soft_unsupported(N, nx, nu, ng)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, why);
        return nullptr;
    }
    std::vector<int> nbs(N + 1);
    for (int k = 0; k <= N; k++) {
        if (nb[k] < 0 || ns[k] < 0) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "soft IPM: nb[k], ns[k] >= 0 required");
            return nullptr;
        }
        nbs[k] = nb[k] + ns[k];
    }
    auto* S = new hpmpc_mi355x_soft_plan();
    S->N = N;
    // the tile path's limits, round_up(nb + ns, 4) <= 16 among them
    S->tile.reset(hpmpc_mi355x_plan_create(N, nx, nu, nbs.data(), idxb, ng));
    if (!S->tile) {
        delete S;
        return nullptr;
    }
    if (const char* why = soft_layout(N, nx, nu, nb, ns, S->L)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, why);
        delete S;
        return nullptr;
    }
    S->mu_scal = soft_mu_scal(N, nb, ns);
    const long long n1 = N + 1;
    auto r8 = [](long long n) { return (n + 7) / 8 * 8; };
    long long o = n1 * FSTRIDE;
    S->oV16 = o;
    o += 7 * n1 * V16;
    S->oCv = o;
    S->nCv = r8(S->L.sC + 1);
    o += 4 * S->nCv;
    S->oFlat = o;
    o += r8(S->L.sF);
    S->oScal = o;
    o += 8;
    S->oIst = o;
    o += 8;
    S->ws = (o + 31) / 32 * 32;  // 256-byte granules: every problem's arrays keep their cache-line alignment
    std::vector<int> idx(n1 * 16, 0);
    idxb_table(N, nbs.data(), idxb, idx.data());
    if (!S->d_st.upload(S->L.st, "soft plan tables") || !S->d_idx.upload(idx, "soft plan tables")) {
        delete S;
        return nullptr;
    }
    g_err = 0;
    return S;
}

// out[6]: doubles per problem of d, Z (= z), lam (= t), ux (= pi), the workspace; N
extern "C" int hpmpc_mi355x_soft_sizes(const hpmpc_mi355x_soft_plan* S, long long* out) {
    if (!S || !out) return HPMPC_MI355X_EUNSUPPORTED;
    const long long v[6] = {S->L.sD, S->L.sZ, S->L.sC, (long long)(S->N + 1) * V16, S->ws, S->N};
    memcpy(out, v, sizeof v);
    return 0;
}

// out[3*(N+1)]: oD, oZ, oC of every stage (doubles inside one problem's d, Z / z, lam / t)
extern "C" int hpmpc_mi355x_soft_offsets(const hpmpc_mi355x_soft_plan* S, long long* out) {
    if (!S || !out) return HPMPC_MI355X_EUNSUPPORTED;
    for (int k = 0; k <= S->N; k++) {
        const SoftStage& s = S->L.st[k];
        out[3 * k] = s.oD;
        out[3 * k + 1] = s.oZ;
        out[3 * k + 2] = s.oC;
    }
    return 0;
}

// d_ip2_mpc_soft_tv on problems [p0, p0 + count) of a device-resident batch.  Asynchronous on `stream`: two launches
// (hk_soft_ipm_init, hk_soft_ipm), no synchronisation (a layout's first use uploads its stage table, batch_args).
extern "C" int hpmpc_mi355x_ipm_soft_batch(const hpmpc_mi355x_soft_plan* S, const hpmpc_mi355x_layout* lay, int nprob,
                                           int p0, int count, const double* BAbt, const double* RSQrq,
                                           const double* Z, const double* z, const double* d, double* ux, double* pi,
                                           double* lam, double* t, double* ws, int k_max, double mu0, double mu_tol,
                                           double alpha_min, int warm_start, int compute_mult, int* kk, int* ret,
                                           double* stat, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ipm_soft_batch";
    if (!range_ok(S, nprob, p0, count, who)) return g_err;
    if (k_max < 0 || !kk || !ret) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ipm_soft_batch: k_max >= 0, kk and ret are required");
        return g_err;
    }
    if (count == 0) return 0;
    hipStream_t st = (hipStream_t)stream;
    if (S->mu_scal == 0.0) {
        // no constraint anywhere: the reference solves into its workspace and leaves every output but kk untouched
        // (d_ip2_soft.c:273-284); kk = 0, ret = 0
        if (!hip_ok(hipMemsetAsync(kk + p0, 0, sizeof(int) * count, st), "memset kk") ||
            !hip_ok(hipMemsetAsync(ret + p0, 0, sizeof(int) * count, st), "memset ret"))
            return g_err;
        return 0;
    }
    const bool soft = S->L.sZ > 0;
    if (!BAbt || !RSQrq || !d || !ux || !pi || !lam || !t || !ws || (k_max > 0 && !stat) || (soft && (!Z || !z)))
        return null_array(who);
    const int N = S->N;
    const long long n1 = N + 1, v16 = n1 * V16;
    KArgs a;
    if (!batch_args(a, S->tile.get(), lay, nprob, p0, DCT_NONE)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ws = ws;
    a.sW = S->ws;
    a.sV16 = S->ws;  // the Riccati vectors live in the workspace
    double* V = ws + S->oV16;
    a.ux = V;  // the Riccati solution: the step's target dux / dpi
    a.pi = V + v16;
    a.vb = V + 2 * v16;
    a.vq = V + 3 * v16;
    a.vQx = V + 4 * v16;
    a.vqx = V + 5 * v16;
    a.vPb = V + 6 * v16;
    soft_ric_flags(a, compute_mult);
    a.k_max = k_max;
    SoftArgs s = soft_scalars(N, nprob, p0, k_max, warm_start, mu0, mu_tol, alpha_min, S->mu_scal);
    s.st = S->d_st.get();
    s.idxb = S->d_idx.get();
    s.d = d;
    s.Z = Z;
    s.z = z;
    s.sD = S->L.sD;
    s.sZ = S->L.sZ;
    s.t = t;
    s.lam = lam;
    s.sC = S->L.sC;
    s.ux = ux;
    s.pi = pi;
    s.sV = v16;
    double* Cv = ws + S->oCv;
    s.dt = Cv;
    s.dlam = Cv + S->nCv;
    s.lamt = Cv + 2 * S->nCv;
    s.tinv = Cv + 3 * S->nCv;
    s.flat = ws + S->oFlat;
    s.dux = V;
    s.dpi = V + v16;
    s.vb = V + 2 * v16;
    s.vq = V + 3 * v16;
    s.vQx = V + 4 * v16;
    s.vqx = V + 5 * v16;
    s.scal = ws + S->oScal;
    s.ist = reinterpret_cast<int*>(ws + S->oIst);
    s.sW = S->ws;
    s.stat = stat;
    s.sS = 5LL * k_max;
    s.kk = kk;
    s.ret = ret;
    if (const int e = hk_soft_ipm_launch(&a, &s, count, st)) return launch_error(e, "hk_soft_ipm launch failed");
    return g_err = 0;
}

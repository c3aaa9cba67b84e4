// hpmpc_capi_ocp.cpp -- the batched OCP front end: the include/c_interface.h wrappers' top layer for a batch whose
// dense problem data (A, B, b, Q, S, R, q, r, lb, ub, C, D, lg, ug) are already in HBM.  hpmpc_mi355x_ocp_pack_batch
// does what pack_problem() of hpmpc_capi_iface.cpp does per problem on the host (hk_ocp_pack, hk_ocp.hip),
// hpmpc_mi355x_ocp_ipm_batch is hpmpc_mi355x_ipm_batch's pass sequence with the DCt array set (so general
// constraints are served here), and hpmpc_mi355x_ocp_finish_batch does what outputs() does: the plain residuals
// (hk_res with res_plain, into a scratch of its own, so the IPM's factor in ws survives) and hk_ocp_unpack, which
// hpmpc_mi355x_ocp_unpack_sets runs without the residual norms for the sets of a multi-set re-solve.
//
// An OCP plan wraps a tile plan -- the lib4 / vector arrays are in its packed default layout -- and the device
// table of stage sizes and dense offsets (OcpStage, hk_ocp_args.h).  Dense arrays: per problem the stage blocks
// concatenated in stage order, column-major or row-major blocks by the plan's flag; per array a problem stride, 0
// for data shared by every problem.  One difference from pack_problem(): RSQrq_k gets S in both triangles, as
// oracle/iface_oracle.py to_qp builds it (pack_problem leaves the upper one zero; every kernel reads the lower).
#include "hk_ocp_plan.h"

extern "C" void hpmpc_mi355x_ocp_plan_destroy(hpmpc_mi355x_ocp_plan* O) { delete O; }

extern "C" hpmpc_mi355x_ocp_plan* hpmpc_mi355x_ocp_plan_create(int N, const int* nx, const int* nu, const int* nb,
                                                               const int* const* idxb, const int* ng, int row_major) {
    g_err = 0;
    if (N < 1 || !nx || !nu || !nb || !ng) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_plan_create: N >= 1 and the size arrays are required");
        return nullptr;
    }
    for (int k = 0; k <= N; k++) {  // check_sizes of the one-problem wrappers (fortran_order_interface.c:106-114)
        const int u = k < N ? nu[k] : 0;
        if (nb[k] > u + nx[k] || (nb[k] > 0 && (!idxb || !idxb[k]))) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_plan_create: nb[k] > nu[k] + nx[k], or no idxb[k]");
            return nullptr;
        }
    }
    auto* O = new hpmpc_mi355x_ocp_plan();
    O->N = N;
    O->row_major = row_major ? 1 : 0;
    O->tile.reset(hpmpc_mi355x_plan_create(N, nx, nu, nb, idxb, ng));  // the tile path's limits
    if (!O->tile) {
        delete O;
        return nullptr;
    }
    const hpmpc_mi355x_plan* P = O->tile.get();
    const long long n1 = N + 1;
    O->st.resize(n1);
    std::vector<int> idx(n1 * 16, 0);
    idxb_table(N, nb, idxb, idx.data());
    long long* D = O->dense;
    for (int k = 0; k <= N; k++) {
        OcpStage& s = O->st[k];
        memset(&s, 0, sizeof s);
        const StageInfoH& h = P->st[k];
        s.nu = h.nu;
        s.nx = h.nx;
        s.nx1 = h.nx1;
        s.nb = h.nb;
        s.ng = h.ng;
        s.pnb = h.pnb;
        s.png = rup(h.ng, BS);
        const int nux = s.nu + s.nx;
        if (k < N)  // outputs(): for (j = 0; j < nb[k] && idxb[k][j] < nu[k]; j++)
            while (s.nbu < s.nb && idxb[k][s.nbu] < s.nu) s.nbu++;
        s.sd[OCP_SEC_BABT] = h.sdB;
        s.sd[OCP_SEC_RSQ] = h.sdR;
        s.sd[OCP_SEC_DCT] = rup(s.ng, NCL);
        s.n[OCP_SEC_BABT] = k < N ? rup(nux + 1, BS) * h.sdB : 0;
        s.n[OCP_SEC_RSQ] = rup(nux + 1, BS) * h.sdR;
        s.n[OCP_SEC_DCT] = s.ng > 0 ? rup(nux, BS) * rup(s.ng, NCL) : 0;
        s.o[OCP_SEC_BABT] = k < N ? (int)P->offB[k] : 0;
        s.o[OCP_SEC_RSQ] = (int)P->offR[k];
        s.o[OCP_SEC_DCT] = (int)P->offG[k];
        for (int i = 0; i < OCP_NARR; i++) s.dn[i] = (int)D[i];
        D[OCP_A] += (long long)s.nx1 * s.nx;
        D[OCP_B] += (long long)s.nx1 * s.nu;
        D[OCP_b] += s.nx1;
        D[OCP_Q] += (long long)s.nx * s.nx;
        D[OCP_S] += (long long)s.nu * s.nx;
        D[OCP_R] += (long long)s.nu * s.nu;
        D[OCP_q] += s.nx;
        D[OCP_r] += s.nu;
        D[OCP_lb] += s.nb;
        D[OCP_ub] += s.nb;
        D[OCP_C] += (long long)s.ng * s.nx;
        D[OCP_D] += (long long)s.ng * s.nu;
        D[OCP_lg] += s.ng;
        D[OCP_ug] += s.ng;
    }
    O->su = D[OCP_r];
    O->sx = D[OCP_q];
    O->sp = D[OCP_b];
    O->sl = 2 * D[OCP_lb] + 2 * D[OCP_lg];
    O->sRes = 2 * n1 * V16 + 2 * n1 * V32;
    if (!O->d_st.upload(O->st, "ocp plan tables") || !O->d_idx.upload(idx, "ocp plan tables")) {
        delete O;
        return nullptr;
    }
    g_err = 0;
    return O;
}

extern "C" const hpmpc_mi355x_plan* hpmpc_mi355x_ocp_tile_plan(const hpmpc_mi355x_ocp_plan* O) {
    return O ? O->tile.get() : nullptr;
}

// out[HPMPC_MI355X_OCP_NSIZES]: doubles per problem, see include/hpmpc_mi355x.h
extern "C" int hpmpc_mi355x_ocp_sizes(const hpmpc_mi355x_ocp_plan* O, long long* out) {
    if (!O || !out) return HPMPC_MI355X_EUNSUPPORTED;
    const long long n1 = O->N + 1;
    for (int i = 0; i < OCP_NARR; i++) out[i] = O->dense[i];
    const long long v[] = {O->tile->packB, O->tile->packR, O->tile->packG, n1 * V32,  n1 * V16, n1 * V16,
                           n1 * V32,       ws_doubles(O->N), O->sRes + 8,   O->su,     O->sx,    O->sp,
                           O->sl,          4,                O->N};
    static_assert(OCP_NARR == HPMPC_MI355X_OCP_NARRAYS && OCP_NARR + 1 + OCP_NSEC == HPMPC_MI355X_OCP_NOFFSETS, "header and kernel tables");
    static_assert(OCP_NARR + sizeof v / sizeof v[0] == HPMPC_MI355X_OCP_NSIZES, "hpmpc_mi355x_ocp_sizes layout");
    memcpy(out + OCP_NARR, v, sizeof v);
    return 0;
}

// out[HPMPC_MI355X_OCP_NOFFSETS * (N+1)]: per stage the offsets of the 14 dense arrays, of the lam / t outputs,
// and of the BAbt_k / RSQrq_k / DCt_k blocks (u / x / pi outputs sit at the offsets of r / q / b)
extern "C" int hpmpc_mi355x_ocp_offsets(const hpmpc_mi355x_ocp_plan* O, long long* out) {
    if (!O || !out) return HPMPC_MI355X_EUNSUPPORTED;
    for (int k = 0; k <= O->N; k++) {
        const OcpStage& s = O->st[k];
        long long v[HPMPC_MI355X_OCP_NOFFSETS];
        for (int i = 0; i < OCP_NARR; i++) v[i] = s.dn[i];
        v[OCP_NARR] = 2LL * s.dn[OCP_lb] + 2LL * s.dn[OCP_lg];
        for (int i = 0; i < OCP_NSEC; i++) v[OCP_NARR + 1 + i] = s.o[i];
        memcpy(out + (long long)HPMPC_MI355X_OCP_NOFFSETS * k, v, sizeof v);
    }
    return 0;
}

extern "C" int hpmpc_mi355x_ocp_pack_batch(const hpmpc_mi355x_ocp_plan* O, const hpmpc_mi355x_ocp_data* data,
                                           int matrices, int nprob, int p0, int count, double* BAbt, double* RSQrq,
                                           double* DCt, double* d, const double* u0, const double* x0, double* ux,
                                           void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_pack_batch";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (count == 0) return 0;
    if (!data || !BAbt || !RSQrq || !d || (O->tile->ngt && !DCt)) return null_array(who);
    OcpPackArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < OCP_NARR; i++) {
        if (O->dense[i] > 0 && !data->ptr[i]) return null_array(who);
        if (data->stride[i] < 0) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_pack_batch: negative stride");
            return g_err;
        }
        a.in[i].p = data->ptr[i];
        a.in[i].s = data->stride[i];
    }
    const long long n1 = O->N + 1;
    a.N = O->N;
    a.nprob = nprob;
    a.p0 = p0;
    a.count = count;
    a.matrices = matrices ? 1 : 0;
    a.row_major = O->row_major;
    a.st = O->d_st.get();
    a.out[OCP_SEC_BABT] = BAbt;
    a.out[OCP_SEC_RSQ] = RSQrq;
    a.out[OCP_SEC_DCT] = DCt;
    a.sout[OCP_SEC_BABT] = O->tile->packB;
    a.sout[OCP_SEC_RSQ] = O->tile->packR;
    a.sout[OCP_SEC_DCT] = O->tile->packG;
    a.d = d;
    a.sV32 = n1 * V32;
    if (ux && (u0 || O->su == 0) && (x0 || O->sx == 0)) {  // the warm start: ux_k = [u0_k | x0_k | 0 ..]
        a.u0 = u0;
        a.x0 = x0;
        a.su = O->su;
        a.sx = O->sx;
        a.ux = ux;
        a.sV16 = n1 * V16;
    }
    if (const int e = hk_ocp_pack_launch(&a, (hipStream_t)stream)) return launch_error(e, "hk_ocp_pack launch failed");
    return g_err = 0;
}

// hpmpc_mi355x_ipm_batch's pass sequence (K_IPM) on the packed default layout with a.DCt set.  mu0 <= 0 is refused:
// the one-problem wrappers then take the problem's largest cost entry, a per-problem value, and the kernels take one
// scalar for the batch.
extern "C" int hpmpc_mi355x_ocp_ipm_batch(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count,
                                          const double* BAbt, const double* RSQrq, const double* DCt, const double* d,
                                          double* ux, double* pi, double* lam, double* t, double* ws, int k_max,
                                          double mu0, double mu_tol, double alpha_min, int warm_start,
                                          int compute_mult, int* kk, int* ret, double* stat, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_ipm_batch";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (!(mu0 > 0.0) || k_max < 0) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_ipm_batch: mu0 > 0 (one value for the batch; the "
                                                "wrappers' cost-based mu0 is per problem) and k_max >= 0");
        return g_err;
    }
    if (count == 0) return 0;
    if (!BAbt || !RSQrq || !d || !ux || !pi || !lam || !t || !ws || !kk || !ret || (k_max > 0 && !stat) ||
        (O->tile->ngt && !DCt))
        return null_array(who);
    KArgs a;  // the tile plan's tables with the packed default layout and the DCt array
    if (!batch_args(a, O->tile.get(), nullptr, nprob, p0, DCT_ARRAY, DCt)) return g_err;
    return ipm_run(a, count, BAbt, RSQrq, d, ux, pi, lam, t, ws, k_max, mu0, mu_tol, alpha_min, warm_start,
                   compute_mult, kk, ret, stat, K_IPM, stream);
}

// hk_ocp_unpack on `nsets` sets per problem of the padded d, ux, pi, lam, t (sV16 / sV32 between sets); res / mu /
// inf set: the finish's residual norms (one set per problem).
static int ocp_unpack(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int nsets, const double* d,
                      const double* ux, const double* pi, const double* lam, const double* t, const OcpOut& out,
                      const double* res, const double* mu, double* inf, void* stream, const char* failed) {
    const long long n1 = O->N + 1;
    OcpUnpackArgs f;
    memset(&f, 0, sizeof f);
    f.N = O->N;
    f.nprob = nprob;
    f.p0 = p0;
    f.count = count;
    f.nsets = nsets;
    f.st = O->d_st.get();
    f.idxb = O->d_idx.get();
    f.d = d;
    f.ux = ux;
    f.pi = pi;
    f.lam = lam;
    f.t = t;
    f.sV16 = n1 * V16;
    f.sV32 = n1 * V32;
    f.out = out;
    f.res = res;
    f.sRes = O->sRes;
    f.mu = mu;
    f.inf = inf;
    if (const int e = hk_ocp_unpack_launch(&f, (hipStream_t)stream)) return launch_error(e, failed);
    return g_err = 0;
}

// res: nprob residual images of 2 (N+1) V16 + 2 (N+1) V32 doubles ([rq | rb | rd | rm], hk_res's ws / sW), then the
// nprob values of mu -- within the nprob * sizes[res] doubles the caller allocates.
extern "C" int hpmpc_mi355x_ocp_finish_batch(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count,
                                             const double* BAbt, const double* RSQrq, const double* DCt,
                                             const double* d, const double* ux, const double* pi, const double* lam,
                                             const double* t, double* res, double* u, double* x, double* pi_out,
                                             double* lam_out, double* t_out, double* inf_norm_res, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_finish_batch";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (count == 0) return 0;
    const OcpOut out = ocp_out(O, u, x, pi_out, lam_out, t_out);
    if (!BAbt || !RSQrq || !d || !ux || !pi || !lam || !t || !res || !inf_norm_res || (O->tile->ngt && !DCt) ||
        !ocp_out_ok(out, false))
        return null_array(who);
    double* mu = res + (long long)nprob * O->sRes;
    KArgs a;
    if (!batch_args(a, O->tile.get(), nullptr, nprob, p0, DCT_ARRAY, DCt)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.d = d;
    a.ux = const_cast<double*>(ux);  // hk_res reads the iterate
    a.pi = const_cast<double*>(pi);
    a.lam = const_cast<double*>(lam);
    a.t = const_cast<double*>(t);
    a.ws = res;
    a.sW = O->sRes;
    a.res_plain = 1;  // d_res_mpc_hard_tv
    a.mu_out = mu;
    if (const int e = hk_launch(K_RES, &a, count, (hipStream_t)stream)) return launch_error(e, "hk_res launch failed");
    return ocp_unpack(O, nprob, p0, count, 1, d, ux, pi, lam, t, out, res, mu, inf_norm_res, stream,
                      "hk_ocp_finish launch failed");
}

// The multi-set finish of re-solved sets: the same placement and equality-box fix (from each set's own d), nrhs
// sets per problem, no residuals.
extern "C" int hpmpc_mi355x_ocp_unpack_sets(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int nrhs,
                                            const double* d, const double* ux, const double* pi, const double* lam,
                                            const double* t, double* u, double* x, double* pi_out, double* lam_out,
                                            double* t_out, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_unpack_sets";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (!sets_ok(nprob, nrhs, "hpmpc_mi355x_ocp_unpack_sets: nrhs")) return g_err;
    if (count == 0) return 0;
    const OcpOut out = ocp_out(O, u, x, pi_out, lam_out, t_out);
    if (!d || !ux || !pi || !lam || !t || !ocp_out_ok(out, false)) return null_array(who);
    return ocp_unpack(O, nprob, p0, count, nrhs, d, ux, pi, lam, t, out, nullptr, nullptr, nullptr, stream,
                      "hk_ocp_unpack_sets launch failed");
}

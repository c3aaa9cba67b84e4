// hpmpc_capi_ocp_soft.cpp -- the batched OCP front end for soft-constrained problems: the top layer of
// fortran_order_d_ip_ocp_soft_tv (hpmpc_capi_iface.cpp) for a batch whose dense problem data (A, B, b, Q, S, R, q, r,
// lb, ub, Z, z) are already in HBM.  hpmpc_mi355x_ocp_soft_pack_batch does what that wrapper's packing loop does per
// problem on the host (hk_ocp_soft_pack / _pack_vec, hk_ocp_soft.hip), hpmpc_mi355x_ocp_soft_ipm_batch is
// hpmpc_mi355x_ipm_soft_batch on the packed default layout, and hpmpc_mi355x_ocp_soft_finish_batch does what the
// wrapper does after the solve: d_res_mpc_soft_tv over the batch (hk_ocp_soft_res, into a scratch of its own) and the
// compact outputs with the residual infinity norms (hk_ocp_soft_unpack).
//
// A soft OCP plan owns a soft plan -- the packed arrays are what hpmpc_mi355x_ipm_soft_batch takes with a null layout
// -- and the device table of stage sizes, dense offsets and soft offsets (OcpSoftStage, hk_ocp_soft_args.h).  One
// difference from the wrapper: a given z is packed and used; the wrapper (like the reference's) leaves z at zero.
#include "hk_ocp_soft_plan.h"

extern "C" void hpmpc_mi355x_ocp_soft_plan_destroy(hpmpc_mi355x_ocp_soft_plan* O) { delete O; }

extern "C" hpmpc_mi355x_ocp_soft_plan* hpmpc_mi355x_ocp_soft_plan_create(int N, const int* nx, const int* nu,
                                                                         const int* nb, const int* const* idxb,
                                                                         const int* ng, const int* ns, int row_major) {
    g_err = 0;
    if (N < 1 || !nx || !nu || !nb || !ng || !ns) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_soft_plan_create: N >= 1 and the size arrays are required");
        return nullptr;
    }
    std::vector<int> nuv(nu, nu + N + 1);
    nuv[N] = 0;  // as the one-problem wrapper and hpmpc_mi355x_ocp_plan_create take it
    for (int k = 0; k <= N; k++) {
        if (nb[k] < 0 || ns[k] < 0 || nb[k] + ns[k] > nuv[k] + nx[k] || (nb[k] + ns[k] > 0 && (!idxb || !idxb[k]))) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED,
                         "hpmpc_mi355x_ocp_soft_plan_create: nb[k] + ns[k] > nu[k] + nx[k], or no idxb[k]");
            return nullptr;
        }
    }
    auto* O = new hpmpc_mi355x_ocp_soft_plan();
    O->N = N;
    O->row_major = row_major ? 1 : 0;
    O->soft.reset(hpmpc_mi355x_soft_plan_create(N, nx, nuv.data(), nb, idxb, ng, ns));  // the soft IPM's limits
    if (!O->soft) {
        delete O;
        return nullptr;
    }
    const hpmpc_mi355x_soft_plan* S = O->soft.get();
    const hpmpc_mi355x_plan* P = S->tile.get();
    const long long n1 = N + 1;
    O->st.resize(n1);
    // the reference's soft residual reads idxb[k][nu_k + i] (d_res_ip_soft.c:107): inside the nb + ns entries only
    // if nu_k <= nb_k on every stage that has soft boxes
    O->res_ok = 1;
    long long* D = O->dense;
    long long olam = 0;
    for (int k = 0; k <= N; k++) {
        OcpSoftStage& s = O->st[k];
        memset(&s, 0, sizeof s);
        const StageInfoH& h = P->st[k];
        const SoftStage& ss = S->L.st[k];
        OcpStage& o = s.o;
        o.nu = h.nu;
        o.nx = h.nx;
        o.nx1 = h.nx1;
        o.nb = ss.nb;
        o.pnb = ss.pnb;
        const int nux = o.nu + o.nx;
        o.sd[OCP_SEC_BABT] = h.sdB;
        o.sd[OCP_SEC_RSQ] = h.sdR;
        o.n[OCP_SEC_BABT] = k < N ? rup(nux + 1, BS) * h.sdB : 0;
        o.n[OCP_SEC_RSQ] = rup(nux + 1, BS) * h.sdR;
        o.o[OCP_SEC_BABT] = k < N ? (int)P->offB[k] : 0;
        o.o[OCP_SEC_RSQ] = (int)P->offR[k];
        for (int i = 0; i <= OCP_ub; i++) o.dn[i] = (int)D[i];
        s.ns = ss.ns;
        s.pns = ss.pns;
        s.oD = ss.oD;
        s.oZ = ss.oZ;
        s.oC = ss.oC;
        s.dnZ = (int)D[OCPS_Z];
        s.olam = (int)olam;
        if (k < N && s.ns > 0 && o.nu > o.nb) O->res_ok = 0;
        D[OCP_A] += (long long)o.nx1 * o.nx;
        D[OCP_B] += (long long)o.nx1 * o.nu;
        D[OCP_b] += o.nx1;
        D[OCP_Q] += (long long)o.nx * o.nx;
        D[OCP_S] += (long long)o.nu * o.nx;
        D[OCP_R] += (long long)o.nu * o.nu;
        D[OCP_q] += o.nx;
        D[OCP_r] += o.nu;
        D[OCP_lb] += o.nb + s.ns;
        D[OCP_ub] += o.nb + s.ns;
        D[OCPS_Z] += 2 * s.ns;
        D[OCPS_z] += 2 * s.ns;
        olam += 2 * o.nb + 4 * s.ns;
    }
    O->su = D[OCP_r];
    O->sx = D[OCP_q];
    O->sp = D[OCP_b];
    O->sl = olam;
    O->sRes = 2 * n1 * V16 + S->L.sD + S->L.sZ;
    if (!O->d_st.upload(O->st, "soft ocp plan tables")) {
        delete O;
        return nullptr;
    }
    g_err = 0;
    return O;
}

extern "C" const hpmpc_mi355x_soft_plan* hpmpc_mi355x_ocp_soft_ipm_plan(const hpmpc_mi355x_ocp_soft_plan* O) {
    return O ? O->soft.get() : nullptr;
}

// out[HPMPC_MI355X_OCP_SOFT_NSIZES]: doubles per problem, see include/hpmpc_mi355x.h
extern "C" int hpmpc_mi355x_ocp_soft_sizes(const hpmpc_mi355x_ocp_soft_plan* O, long long* out) {
    if (!O || !out) return HPMPC_MI355X_EUNSUPPORTED;
    const hpmpc_mi355x_soft_plan* S = O->soft.get();
    const long long n1 = O->N + 1;
    for (int i = 0; i < OCPS_NARR; i++) out[i] = O->dense[i];
    const long long v[] = {S->tile->packB, S->tile->packR, S->L.sD, S->L.sZ, n1 * V16, S->L.sC, S->ws, O->sRes + 8,
                           O->su,          O->sx,          O->sp,   O->sl,   4,        O->res_ok, O->N};
    static_assert(OCPS_NARR == HPMPC_MI355X_OCP_SOFT_NARRAYS, "header and kernel tables");
    static_assert(OCPS_NARR + sizeof v / sizeof v[0] == HPMPC_MI355X_OCP_SOFT_NSIZES, "hpmpc_mi355x_ocp_soft_sizes layout");
    memcpy(out + OCPS_NARR, v, sizeof v);
    return 0;
}

// out[HPMPC_MI355X_OCP_SOFT_NOFFSETS * (N+1)]: per stage the offsets of the 12 dense arrays, of the lam / t outputs,
// of the BAbt_k / RSQrq_k blocks and of d_k, Z_k / z_k, lam_k / t_k (u / x / pi outputs sit at the offsets of r / q / b)
extern "C" int hpmpc_mi355x_ocp_soft_offsets(const hpmpc_mi355x_ocp_soft_plan* O, long long* out) {
    if (!O || !out) return HPMPC_MI355X_EUNSUPPORTED;
    for (int k = 0; k <= O->N; k++) {
        const OcpSoftStage& s = O->st[k];
        long long v[HPMPC_MI355X_OCP_SOFT_NOFFSETS];
        for (int i = 0; i <= OCP_ub; i++) v[i] = s.o.dn[i];
        v[OCPS_Z] = v[OCPS_z] = s.dnZ;
        const long long w[] = {s.olam, s.o.o[OCP_SEC_BABT], s.o.o[OCP_SEC_RSQ], s.oD, s.oZ, s.oC};
        static_assert(OCPS_NARR + sizeof w / sizeof w[0] == HPMPC_MI355X_OCP_SOFT_NOFFSETS, "hpmpc_mi355x_ocp_soft_offsets layout");
        memcpy(v + OCPS_NARR, w, sizeof w);
        memcpy(out + (long long)HPMPC_MI355X_OCP_SOFT_NOFFSETS * k, v, sizeof v);
    }
    return 0;
}

extern "C" int hpmpc_mi355x_ocp_soft_pack_batch(const hpmpc_mi355x_ocp_soft_plan* O,
                                                const hpmpc_mi355x_ocp_soft_data* data, int matrices, int nprob, int p0,
                                                int count, double* BAbt, double* RSQrq, double* d, double* Z, double* z,
                                                const double* u0, const double* x0, double* ux, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_soft_pack_batch";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (count == 0) return 0;
    const hpmpc_mi355x_soft_plan* S = O->soft.get();
    if (!data || !BAbt || !RSQrq || (S->L.sD > 0 && !d) || (S->L.sZ > 0 && (!Z || !z))) return null_array(who);
    OcpSoftPackArgs a;
    memset(&a, 0, sizeof a);
    for (int i = 0; i < OCPS_NARR; i++) {
        if (i != OCPS_z && O->dense[i] > 0 && !data->ptr[i]) return null_array(who);  // a null z packs zeros
        if (data->stride[i] < 0) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_soft_pack_batch: negative stride");
            return g_err;
        }
        a.in[i].p = data->ptr[i];
        a.in[i].s = data->stride[i];
    }
    a.N = O->N;
    a.nprob = nprob;
    a.p0 = p0;
    a.count = count;
    a.matrices = matrices ? 1 : 0;
    a.row_major = O->row_major;
    a.st = O->d_st.get();
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.sB = S->tile->packB;
    a.sR = S->tile->packR;
    a.d = d;
    a.Z = Z;
    a.z = z;
    a.sD = S->L.sD;
    a.sZ = S->L.sZ;
    if (ux && (u0 || O->su == 0) && (x0 || O->sx == 0)) {  // the warm start: ux_k = [u0_k | x0_k | 0 ..]
        a.u0 = u0;
        a.x0 = x0;
        a.su = O->su;
        a.sx = O->sx;
        a.ux = ux;
        a.sV16 = (long long)(O->N + 1) * V16;
    }
    if (const int e = hk_ocp_soft_pack_launch(&a, (hipStream_t)stream)) return launch_error(e, "hk_ocp_soft_pack launch failed");
    return g_err = 0;
}

// hpmpc_mi355x_ipm_soft_batch on the packed default layout.  mu0 <= 0 is refused: the one-problem wrapper then takes
// the problem's largest cost entry, a per-problem value, and the kernel takes one scalar for the batch.
extern "C" int hpmpc_mi355x_ocp_soft_ipm_batch(const hpmpc_mi355x_ocp_soft_plan* O, int nprob, int p0, int count,
                                               const double* BAbt, const double* RSQrq, const double* Z,
                                               const double* z, const double* d, double* ux, double* pi, double* lam,
                                               double* t, double* ws, int k_max, double mu0, double mu_tol,
                                               double alpha_min, int warm_start, int compute_mult, int* kk, int* ret,
                                               double* stat, void* stream) {
    g_err = 0;
    if (!range_ok(O, nprob, p0, count, "hpmpc_mi355x_ocp_soft_ipm_batch")) return g_err;
    if (!(mu0 > 0.0)) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_soft_ipm_batch: mu0 > 0 (one value for the batch; the "
                                                "wrapper's cost-based mu0 is per problem)");
        return g_err;
    }
    return hpmpc_mi355x_ipm_soft_batch(O->soft.get(), nullptr, nprob, p0, count, BAbt, RSQrq, Z, z, d, ux, pi, lam, t,
                                       ws, k_max, mu0, mu_tol, alpha_min, warm_start, compute_mult, kk, ret, stat,
                                       stream);
}

// res: nprob residual images of sRes doubles ([r_q | r_b] 16 per stage, r_d like d, r_z like Z), then the nprob
// values of mu -- within the nprob * sizes[res] doubles the caller allocates.
extern "C" int hpmpc_mi355x_ocp_soft_finish_batch(const hpmpc_mi355x_ocp_soft_plan* O, int nprob, int p0, int count,
                                                  const double* BAbt, const double* RSQrq, const double* Z,
                                                  const double* z, const double* d, const double* ux,
                                                  const double* pi, const double* lam, const double* t, double* res,
                                                  double* u, double* x, double* pi_out, double* lam_out,
                                                  double* t_out, double* inf_norm_res, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_soft_finish_batch";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (inf_norm_res && !O->res_ok) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_soft_finish_batch: the reference's soft residual reads "
                                                "idxb[k][nu + i] outside idxb[k] on this plan (res_ok = 0)");
        return g_err;
    }
    if (count == 0) return 0;
    const hpmpc_mi355x_soft_plan* S = O->soft.get();
    const OcpOut out = soft_out(O, u, x, pi_out, lam_out, t_out);
    if (!ux || !pi || (S->L.sC > 0 && (!lam || !t)) || !soft_out_ok(out)) return null_array(who);
    const long long n1 = O->N + 1;
    double* mu = nullptr;
    if (inf_norm_res) {
        if (!BAbt || !RSQrq || !res || (S->L.sD > 0 && !d) || (S->L.sZ > 0 && (!Z || !z))) return null_array(who);
        mu = res + (long long)nprob * O->sRes;
        OcpSoftResArgs r;
        memset(&r, 0, sizeof r);
        r.N = O->N;
        r.nprob = nprob;
        r.p0 = p0;
        r.count = count;
        r.st = O->d_st.get();
        r.idxb = S->d_idx.get();
        r.BAbt = BAbt;
        r.RSQ = RSQrq;
        r.d = d;
        r.Z = Z;
        r.z = z;
        r.ux = ux;
        r.pi = pi;
        r.lam = lam;
        r.t = t;
        r.sB = S->tile->packB;
        r.sR = S->tile->packR;
        r.sD = S->L.sD;
        r.sZ = S->L.sZ;
        r.sC = S->L.sC;
        r.sV16 = n1 * V16;
        r.res = res;
        r.sRes = O->sRes;
        r.mu = mu;
        if (const int e = hk_ocp_soft_res_launch(&r, (hipStream_t)stream)) return launch_error(e, "hk_ocp_soft_res launch failed");
    }
    OcpSoftUnpackArgs f;
    memset(&f, 0, sizeof f);
    f.N = O->N;
    f.nprob = nprob;
    f.p0 = p0;
    f.count = count;
    f.st = O->d_st.get();
    f.ux = ux;
    f.pi = pi;
    f.lam = lam;
    f.t = t;
    f.sV16 = n1 * V16;
    f.sC = S->L.sC;
    f.out = out;
    f.res = inf_norm_res ? res : nullptr;
    f.sRes = O->sRes;
    f.mu = mu;
    f.inf = inf_norm_res;
    if (const int e = hk_ocp_soft_unpack_launch(&f, (hipStream_t)stream)) return launch_error(e, "hk_ocp_soft_unpack launch failed");
    return g_err = 0;
}

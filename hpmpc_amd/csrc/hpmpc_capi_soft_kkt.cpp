// hpmpc_capi_soft_kkt.cpp -- the batched KKT re-solve for soft-constrained batches, many right-hand-side sets per factor:
// hpmpc_mi355x_soft_kkt_batch on a soft plan's padded arrays and hpmpc_mi355x_soft_kkt_ocp_batch on the dense per-set
// vectors of the soft OCP front end (hk_soft_kkt.hip).  The reference has no d_kkt_solve_new_rhs_* for its soft IPM;
// include/hpmpc_mi355x.h and DESIGN.md §3d define what the calls compute.
//
// The linearisation (lamt, tinv, Zl, the Riccati factor) sits in the workspace of hpmpc_mi355x_ipm_soft_batch
// (hpmpc_capi_soft_batch.cpp holds its carve): refactor = 0 reads what the last iteration of a solve left there,
// refactor = 1 first rebuilds it at a given (lam, t).  The set launch only reads the workspace; each set's work vectors
// live in the caller's scratch (soft_kkt_scratch_doubles, hk_soft_kkt_args.h).
#include "hk_ocp_soft_plan.h"
#include "hk_soft_kkt_args.h"

extern "C" long long hpmpc_mi355x_soft_kkt_scratch_doubles(const hpmpc_mi355x_soft_plan* S) {
    return S ? soft_kkt_scratch_doubles(S->N) : 0;
}

namespace {

// A set's block of the OCP call's work buffer (OcpSoftKktPackArgs): offsets and size in doubles
struct WorkCarve {
    long long b, q, ux, pi, d, z, lam, t, total;
};
WorkCarve work_carve(const hpmpc_mi355x_soft_plan* S) {
    const long long n16 = (long long)(S->N + 1) * V16;
    WorkCarve w;
    w.b = 0;
    w.q = n16;
    w.ux = 2 * n16;
    w.pi = 3 * n16;
    w.d = 4 * n16;
    w.z = w.d + S->L.sD;
    w.lam = w.z + S->L.sZ;
    w.t = w.lam + S->L.sC;
    w.total = (w.t + S->L.sC + 31) / 32 * 32;  // 256-byte granules: every set's vectors keep their alignment
    return w;
}

// The checks and the launches of both calls.  The per-set arrays come with their strides between sets.
struct SetArrays {
    const double *b, *q, *d, *z;
    double *ux, *pi, *lam, *t;
    long long s16, sD, sZ, sC;
};

int soft_kkt(const hpmpc_mi355x_soft_plan* S, const hpmpc_mi355x_layout* lay, int nprob, int p0, int count, int nrhs,
             const double* BAbt, const double* RSQrq, const double* Z, const double* z0, const double* lam0,
             const double* t0, const SetArrays& v, double* ws, double* scratch, int refactor, int compute_mult,
             void* stream, const char* who) {
    const bool soft = S->L.sZ > 0;
    if (S->mu_scal == 0.0) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x soft re-solve: no constraint on any stage (the ric_*_batch "
                                                "calls solve such problems)");
        return g_err;
    }
    if (!BAbt || !RSQrq || !v.b || !v.q || !v.d || !v.ux || !v.pi || !v.lam || !v.t || !ws || !scratch ||
        (soft && (!Z || (!v.z && !z0))) || (refactor && (!lam0 || !t0)))
        return null_array(who);
    KArgs a;
    if (!batch_args(a, S->tile.get(), lay, nprob, p0, DCT_NONE)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ws = ws;
    a.sW = S->ws;
    a.sV16 = v.s16;
    a.vb = v.b;
    a.vq = v.q;
    a.ux = v.ux;
    a.pi = v.pi;
    a.compute_mult = compute_mult;
    SoftKktArgs x;
    memset(&x, 0, sizeof x);
    x.nrhs = nrhs;
    x.nq = (S->N + 4) / 4;
    x.st = S->d_st.get();
    x.idxb = S->d_idx.get();
    x.Z = Z;
    x.z0 = z0;
    x.sZ = S->L.sZ;
    x.lam0 = lam0;
    x.t0 = t0;
    x.sC = S->L.sC;
    x.d = v.d;
    x.z = v.z;
    x.sDs = v.sD;
    x.sZs = v.sZ;
    x.lam = v.lam;
    x.t = v.t;
    x.sCs = v.sC;
    // the carve of hpmpc_mi355x_soft_plan_create: seven V16 vectors (Qx the fifth), then dt dlam lamt tinv
    x.oVQx = S->oV16 + 4LL * (S->N + 1) * V16;
    x.oLamt = S->oCv + 2 * S->nCv;
    x.oTinv = S->oCv + 3 * S->nCv;
    x.oFlat = S->oFlat;
    x.scratch = scratch;
    x.sS = soft_kkt_scratch_doubles(S->N);
    if (const int e = hk_soft_kkt_launch(&a, &x, count, refactor ? 1 : 0, (hipStream_t)stream))
        return launch_error(e, "hk_soft_kkt launch failed");
    return g_err = 0;
}

}  // namespace

extern "C" int hpmpc_mi355x_soft_kkt_batch(const hpmpc_mi355x_soft_plan* S, const hpmpc_mi355x_layout* lay, int nprob,
                                           int p0, int count, int nrhs, const double* BAbt, const double* RSQrq,
                                           const double* Z, const double* z0, const double* lam0, const double* t0,
                                           const double* b, const double* q, const double* d, const double* z,
                                           double* ux, double* pi, double* lam, double* t, double* ws, double* scratch,
                                           int refactor, int compute_mult, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_soft_kkt_batch";
    if (!range_ok(S, nprob, p0, count, who) || !sets_ok(nprob, nrhs, "hpmpc_mi355x_soft_kkt_batch: nrhs") || count == 0)
        return g_err;
    const long long n16 = (long long)(S->N + 1) * V16;
    const SetArrays v{b, q, d, z, ux, pi, lam, t, n16, S->L.sD, S->L.sZ, S->L.sC};
    return soft_kkt(S, lay, nprob, p0, count, nrhs, BAbt, RSQrq, Z, z0, lam0, t0, v, ws, scratch, refactor, compute_mult,
                    stream, who);
}

extern "C" long long hpmpc_mi355x_soft_kkt_ocp_work_doubles(const hpmpc_mi355x_ocp_soft_plan* O) {
    return O ? work_carve(O->soft.get()).total : 0;
}

// Three launches: the vector pack per set into the work buffer, the call above on the packed default layout, and the
// soft finish's unpack with a set in a problem's place.  Every check comes before the first launch.
extern "C" int hpmpc_mi355x_soft_kkt_ocp_batch(const hpmpc_mi355x_ocp_soft_plan* O, int nprob, int p0, int count,
                                               int nrhs, const double* BAbt, const double* RSQrq, const double* Z,
                                               const double* z0, const double* lam0, const double* t0, const double* b,
                                               const double* q, const double* r, const double* lb, const double* ub,
                                               const double* z, double* u, double* x, double* pi_out, double* lam_out,
                                               double* t_out, double* ws, double* work, double* scratch, int refactor,
                                               void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_soft_kkt_ocp_batch";
    if (!range_ok(O, nprob, p0, count, who) || !sets_ok(nprob, nrhs, "hpmpc_mi355x_soft_kkt_ocp_batch: nrhs") ||
        count == 0)
        return g_err;
    const hpmpc_mi355x_soft_plan* S = O->soft.get();
    const OcpOut out = soft_out(O, u, x, pi_out, lam_out, t_out);
    const long long* D = O->dense;
    if (!work || !soft_out_ok(out) || (D[OCP_b] > 0 && !b) || (D[OCP_q] > 0 && !q) || (D[OCP_r] > 0 && !r) ||
        (D[OCP_lb] > 0 && (!lb || !ub)))
        return null_array(who);
    const WorkCarve w = work_carve(S);
    OcpSoftKktPackArgs pk;
    memset(&pk, 0, sizeof pk);
    pk.N = O->N;
    pk.nprob = nprob;
    pk.p0 = p0;
    pk.count = count;
    pk.nrhs = nrhs;
    pk.st = O->d_st.get();
    pk.b = b;
    pk.q = q;
    pk.r = r;
    pk.lb = lb;
    pk.ub = ub;
    pk.z = D[OCPS_z] > 0 ? z : nullptr;
    pk.nb_ = D[OCP_b];
    pk.nq_ = D[OCP_q];
    pk.nr_ = D[OCP_r];
    pk.nl_ = D[OCP_lb];
    pk.nz_ = D[OCPS_z];
    pk.work = work;
    pk.sWk = w.total;
    pk.oD = w.d;
    pk.oZ = w.z;
    // the re-solve's own checks, before the pack is issued
    if (S->mu_scal == 0.0 || !BAbt || !RSQrq || !ws || !scratch || (S->L.sZ > 0 && (!Z || (!pk.z && !z0))) ||
        (refactor && (!lam0 || !t0))) {
        if (S->mu_scal == 0.0)
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x soft re-solve: no constraint on any stage (the "
                                                    "ric_*_batch calls solve such problems)");
        else
            null_array(who);
        return g_err;
    }
    if (const int e = hk_ocp_soft_kkt_pack_launch(&pk, (hipStream_t)stream))
        return launch_error(e, "hk_ocp_soft_kkt_pack launch failed");
    const SetArrays v{work + w.b, work + w.q, work + w.d, pk.z ? work + w.z : nullptr, work + w.ux, work + w.pi,
                      work + w.lam, work + w.t, w.total, w.total, w.total, w.total};
    if (soft_kkt(S, nullptr, nprob, p0, count, nrhs, BAbt, RSQrq, Z, z0, lam0, t0, v, ws, scratch, refactor, 1, stream,
                 who))
        return g_err;
    OcpSoftUnpackArgs f;  // the sets as the problems of hk_ocp_soft_unpack
    memset(&f, 0, sizeof f);
    f.N = O->N;
    f.nprob = nprob * nrhs;
    f.p0 = p0 * nrhs;
    f.count = count * nrhs;
    f.st = O->d_st.get();
    f.ux = work + w.ux;
    f.pi = work + w.pi;
    f.lam = work + w.lam;
    f.t = work + w.t;
    f.sV16 = f.sC = w.total;
    f.out = out;
    if (const int e = hk_ocp_soft_unpack_launch(&f, (hipStream_t)stream))
        return launch_error(e, "hk_ocp_soft_unpack launch failed");
    return g_err = 0;
}

// hpmpc_capi_tan.cpp -- the batched KKT tangent solve: hpmpc_mi355x_kkt_tangent_batch (padded directions and results,
// the layouts of hpmpc_mi355x_kkt_new_rhs_batch) and hpmpc_mi355x_ocp_tangent_batch (dense directions and results on
// an OCP plan), both one launch of hk_kkt_tan (hk_tan.hip), ndir direction sets per problem; and the multi-set finish
// hpmpc_mi355x_ocp_unpack_sets (hk_ocp_unpack_sets).  The workspaces an IPM left are read only, as in the re-solve
// (hpmpc_capi_kkt.cpp), whose scratch size and refusals these calls share.
#include <climits>

#include "hk_ocp_plan.h"
#include "hk_tan_args.h"

namespace {

// The checks and the argument blocks the two tangent calls share; false: g_err set, nothing launched.  *empty: the
// range holds no problem and the call returns 0 without asking for any array.
bool tan_args(KArgs& a, TanArgs& x, const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob, int p0,
              int count, int ndir, const double* BAbt, const double* RSQrq, const double* DCt, const double* ws,
              double* scratch, int compute_mult, const char* who, bool* empty) {
    *empty = false;
    if (!range_ok(plan, nprob, p0, count, who)) return false;
    // the grid is count * ndir workgroups and a set index is an int
    if (ndir < 1 || (long long)nprob * ndir > INT_MAX) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x tangent call: ndir");
        return false;
    }
    if (count == 0) {
        *empty = true;
        return true;
    }
    if (!BAbt || !RSQrq || !ws || !scratch || (plan->ngt && !DCt)) {
        null_array(who);
        return false;
    }
    if (!batch_args(a, plan, lay, nprob, p0, DCT_ARRAY, DCt)) return false;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ws = const_cast<double*>(ws);  // hk_kkt_tan only reads it
    a.compute_mult = compute_mult;
    memset(&x, 0, sizeof x);
    x.ndir = ndir;
    x.scratch = scratch;
    x.sS = kkt_scratch_doubles(plan->N);
    return true;
}

}  // namespace

extern "C" int hpmpc_mi355x_kkt_tangent_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                              int p0, int count, int ndir, const double* BAbt, const double* RSQrq,
                                              const double* DCt, const double* db, const double* dq, const double* dd,
                                              double* dux, double* dpi, double* dlam, double* dt, const double* ws,
                                              double* scratch, int compute_mult, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_kkt_tangent_batch";
    KArgs a;
    TanArgs x;
    bool empty;
    if (!tan_args(a, x, plan, lay, nprob, p0, count, ndir, BAbt, RSQrq, DCt, ws, scratch, compute_mult, who, &empty))
        return g_err;
    if (empty) return 0;
    if (!dux || !dpi || !dlam || !dt) return null_array(who);
    // the per-set arrays: batch_args' sV16 / sV32 are the strides between sets; a null direction is zero
    a.vb = db;
    a.vq = dq;
    a.d = dd;
    a.ux = dux;
    a.pi = dpi;
    a.lam = dlam;
    a.t = dt;
    if (const int e = hk_kkt_tan_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_tan launch failed");
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ocp_tangent_batch(const hpmpc_mi355x_ocp_plan* O, const hpmpc_mi355x_ocp_data* dirs,
                                              int nprob, int p0, int count, int ndir, const double* BAbt,
                                              const double* RSQrq, const double* DCt, double* du, double* dx,
                                              double* dpi, double* dlam, double* dt, const double* ws, double* scratch,
                                              int compute_mult, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_tangent_batch";
    if (!O) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_tangent_batch: plan");
        return g_err;
    }
    KArgs a;
    TanArgs x;
    bool empty;
    if (!tan_args(a, x, O->tile.get(), nullptr, nprob, p0, count, ndir, BAbt, RSQrq, DCt, ws, scratch, compute_mult,
                  who, &empty))
        return g_err;
    if (empty) return 0;
    if (!dirs || (O->su > 0 && !du) || (O->sx > 0 && !dx) || (O->sp > 0 && !dpi) || (O->sl > 0 && (!dlam || !dt)))
        return null_array(who);
    for (int i = 0; i < OCP_NARR; i++) {
        const bool vec = i == OCP_b || i == OCP_q || i == OCP_r || i == OCP_lb || i == OCP_ub || i == OCP_lg ||
                         i == OCP_ug;
        if (!vec && dirs->ptr[i]) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_tangent_batch: matrix directions (A, B, Q, S, R, "
                                                    "C, D) are not supported");
            return g_err;
        }
        if (vec && dirs->ptr[i] && dirs->stride[i] < 0) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_tangent_batch: negative stride");
            return g_err;
        }
        if (vec && O->dense[i] > 0) {  // a vector the plan has no element of is never read
            x.in[i].p = dirs->ptr[i];
            x.in[i].s = dirs->stride[i];
        }
    }
    x.ost = O->d_st.get();
    x.du = du;
    x.dx = dx;
    x.dpo = dpi;
    x.dlo = dlam;
    x.dto = dt;
    x.su = O->su;
    x.sx = O->sx;
    x.sp = O->sp;
    x.sl = O->sl;
    if (const int e = hk_kkt_tan_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_tan launch failed");
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ocp_unpack_sets(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int nrhs,
                                            const double* d, const double* ux, const double* pi, const double* lam,
                                            const double* t, double* u, double* x, double* pi_out, double* lam_out,
                                            double* t_out, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_ocp_unpack_sets";
    if (!range_ok(O, nprob, p0, count, who)) return g_err;
    if (nrhs < 1 || (long long)nprob * nrhs > INT_MAX) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_unpack_sets: nrhs");
        return g_err;
    }
    if (count == 0) return 0;
    if (!d || !ux || !pi || !lam || !t || (O->su > 0 && !u) || (O->sx > 0 && !x) || (O->sp > 0 && !pi_out) ||
        (O->sl > 0 && !lam_out))
        return null_array(who);
    const long long n1 = O->N + 1;
    OcpSetsArgs f;
    memset(&f, 0, sizeof f);
    f.N = O->N;
    f.nprob = nprob;
    f.p0 = p0;
    f.count = count;
    f.nrhs = nrhs;
    f.st = O->d_st.get();
    f.idxb = O->d_idx.get();
    f.d = d;
    f.ux = ux;
    f.pi = pi;
    f.lam = lam;
    f.t = t;
    f.sV16 = n1 * V16;
    f.sV32 = n1 * V32;
    f.u = u;
    f.x = x;
    f.po = pi_out;
    f.lamo = lam_out;
    f.to = t_out;
    f.su = O->su;
    f.sx = O->sx;
    f.sp = O->sp;
    f.sl = O->sl;
    if (const int e = hk_ocp_unpack_sets_launch(&f, (hipStream_t)stream))
        return launch_error(e, "hk_ocp_unpack_sets launch failed");
    return g_err = 0;
}

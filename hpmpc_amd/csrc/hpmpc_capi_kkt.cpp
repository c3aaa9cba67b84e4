// hpmpc_capi_kkt.cpp -- the batched KKT re-solve: hpmpc_mi355x_kkt_new_rhs_batch and hpmpc_mi355x_ocp_kkt_batch,
// d_kkt_solve_new_rhs_res_mpc_hard_tv (mpc_solvers/d_ip2_res_hard.c:1922-2299) on device-resident batches, nrhs
// right-hand-side sets per problem in one launch of hk_kkt_rhs (hk_kkt.hip).  The workspaces an IPM left
// (hpmpc_mi355x_ipm_batch, _ipm_solo, _ocp_ipm_batch) are read only; each set's work vectors live in the caller's
// scratch (kkt_scratch_doubles, hk_kkt_args.h).  The core call carries a DCt array, so it takes tile plans with
// general constraints (batch_args with DCT_ARRAY).
#include <climits>

#include "hk_kkt_args.h"
#include "hk_plan.h"

extern "C" long long hpmpc_mi355x_kkt_scratch_doubles(const hpmpc_mi355x_plan* P) {
    return P ? kkt_scratch_doubles(P->N) : 0;
}

extern "C" int hpmpc_mi355x_kkt_new_rhs_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                              int p0, int count, int nrhs, const double* BAbt, const double* RSQrq,
                                              const double* DCt, const double* b, const double* q, const double* d,
                                              double* ux, double* pi, double* lam, double* t, const double* ws,
                                              double* scratch, int compute_mult, void* stream) {
    g_err = 0;
    const char* who = "hpmpc_mi355x_kkt_new_rhs_batch";
    if (!range_ok(plan, nprob, p0, count, who)) return g_err;
    // the grid is count * nrhs workgroups and a set index is an int
    if (nrhs < 1 || (long long)nprob * nrhs > INT_MAX) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_kkt_new_rhs_batch: nrhs");
        return g_err;
    }
    if (count == 0) return 0;
    if (!BAbt || !RSQrq || !d || !ux || !pi || !lam || !t || !ws || !scratch || (plan->ngt && !DCt))
        return null_array(who);
    KArgs a;
    if (!batch_args(a, plan, lay, nprob, p0, DCT_ARRAY, DCt)) return g_err;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ws = const_cast<double*>(ws);  // hk_kkt_rhs only reads it
    // the per-set arrays: batch_args' sV16 / sV32 are the strides between sets
    a.vb = b;
    a.vq = q;
    a.d = d;
    a.ux = ux;
    a.pi = pi;
    a.lam = lam;
    a.t = t;
    a.compute_mult = compute_mult;
    KktArgs x;
    memset(&x, 0, sizeof x);
    x.nrhs = nrhs;
    x.scratch = scratch;
    x.sS = kkt_scratch_doubles(plan->N);
    if (const int e = hk_kkt_rhs_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_rhs launch failed");
    return g_err = 0;
}

// The batched fortran_order_ / c_order_d_solve_kkt_new_rhs_ocp_hard_tv core: one set per problem, b and q from the
// augmented rows hpmpc_mi355x_ocp_pack_batch(matrices = 0) rewrote, on the packed default layout.
extern "C" int hpmpc_mi355x_ocp_kkt_batch(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count,
                                          const double* BAbt, const double* RSQrq, const double* DCt, const double* d,
                                          double* ux, double* pi, double* lam, double* t, const double* ws,
                                          double* scratch, void* stream) {
    const hpmpc_mi355x_plan* P = hpmpc_mi355x_ocp_tile_plan(O);
    if (!P) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_kkt_batch: plan");
        return g_err;
    }
    return hpmpc_mi355x_kkt_new_rhs_batch(P, nullptr, nprob, p0, count, 1, BAbt, RSQrq, DCt, nullptr, nullptr, d, ux,
                                          pi, lam, t, ws, scratch, 1, stream);
}

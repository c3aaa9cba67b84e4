// hpmpc_capi_kkt.cpp -- the batched calls on the factor an IPM left, many sets per problem in one launch: the KKT
// re-solve hpmpc_mi355x_kkt_new_rhs_batch and hpmpc_mi355x_ocp_kkt_batch, d_kkt_solve_new_rhs_res_mpc_hard_tv
// (mpc_solvers/d_ip2_res_hard.c:1922-2299) on device-resident batches, nrhs right-hand-side sets per problem
// (hk_kkt_rhs, hk_kkt.hip); and its linear part, the KKT tangent solve hpmpc_mi355x_kkt_tangent_batch (padded
// directions and results, the re-solve's layouts) and hpmpc_mi355x_ocp_tangent_batch (dense directions and results on
// an OCP plan), ndir direction sets per problem (hk_kkt_tan, hk_tan.hip); and that tangent's transpose, the KKT adjoint
// solve hpmpc_mi355x_kkt_adjoint_batch / hpmpc_mi355x_ocp_adjoint_batch, nadj cotangent sets per problem (hk_kkt_adj,
// hk_adj.hip), and on its solution the gradients with respect to the dense matrices,
// hpmpc_mi355x_ocp_matrix_grads_batch / hpmpc_mi355x_ocp_adjoint_data_batch (hk_ocp_matgrad, hk_matgrad.hip), and
// forward the seed rows of directions in all fourteen dense arrays, hpmpc_mi355x_ocp_matrix_dirs_batch, and the tangent
// solve on them, hpmpc_mi355x_ocp_tangent_data_batch (hk_ocp_matdir, hk_matdir.hip, then hk_kkt_tan).  The
// workspaces an IPM left (hpmpc_mi355x_ipm_batch, _ipm_solo, _ocp_ipm_batch) are read only; each set's work vectors
// live in the caller's scratch (kkt_scratch_doubles, hk_kkt_args.h).  The core calls carry a DCt array, so they take
// tile plans with general constraints (batch_args with DCT_ARRAY).
#include "hk_adj_args.h"
#include "hk_matdir_args.h"
#include "hk_matgrad_args.h"
#include "hk_ocp_plan.h"
#include "hk_tan_args.h"

extern "C" long long hpmpc_mi355x_kkt_scratch_doubles(const hpmpc_mi355x_plan* P) {
    return P ? kkt_scratch_doubles(P->N) : 0;
}

namespace {

constexpr bool ocp_is_vector(int i) {
    return i == OCP_b || i == OCP_q || i == OCP_r || i == OCP_lb || i == OCP_ub || i == OCP_lg || i == OCP_ug;
}

// A call on an OCP plan without one: true, g_err set with the message `who`.
bool no_plan(const void* O, const char* who) {
    if (O) return false;
    hk_set_error(HPMPC_MI355X_EUNSUPPORTED, who);
    return true;
}

// The checks and the argument blocks these calls share.  arrays: the caller's own required arrays are all there.
// False: nothing to launch, g_err holds the call's return (an error, or 0 for a range without a problem).
bool sets_args(KArgs& a, KktArgs& x, const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob, int p0,
               int count, int nsets, const double* BAbt, const double* RSQrq, const double* DCt, const double* ws,
               double* scratch, bool arrays, int compute_mult, const char* who, const char* sets_msg) {
    g_err = 0;
    if (!range_ok(plan, nprob, p0, count, who) || !sets_ok(nprob, nsets, sets_msg) || count == 0) return false;
    if (!BAbt || !RSQrq || !ws || !scratch || !arrays || (plan->ngt && !DCt)) {
        null_array(who);
        return false;
    }
    if (!batch_args(a, plan, lay, nprob, p0, DCT_ARRAY, DCt)) return false;
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ws = const_cast<double*>(ws);  // the kernels only read it
    a.compute_mult = compute_mult;
    memset(&x, 0, sizeof x);
    x.nrhs = nsets;
    x.scratch = scratch;
    x.sS = kkt_scratch_doubles(plan->N);
    return true;
}

// the per-set arrays: batch_args' sV16 / sV32 are the strides between sets
void set_arrays(KArgs& a, const double* b, const double* q, const double* d, double* ux, double* pi, double* lam,
                double* t) {
    a.vb = b;
    a.vq = q;
    a.d = d;
    a.ux = ux;
    a.pi = pi;
    a.lam = lam;
    a.t = t;
}

}  // namespace

extern "C" int hpmpc_mi355x_kkt_new_rhs_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                              int p0, int count, int nrhs, const double* BAbt, const double* RSQrq,
                                              const double* DCt, const double* b, const double* q, const double* d,
                                              double* ux, double* pi, double* lam, double* t, const double* ws,
                                              double* scratch, int compute_mult, void* stream) {
    KArgs a;
    KktArgs x;
    if (!sets_args(a, x, plan, lay, nprob, p0, count, nrhs, BAbt, RSQrq, DCt, ws, scratch, d && ux && pi && lam && t,
                   compute_mult, "hpmpc_mi355x_kkt_new_rhs_batch", "hpmpc_mi355x_kkt_new_rhs_batch: nrhs"))
        return g_err;
    set_arrays(a, b, q, d, ux, pi, lam, t);
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
    if (no_plan(O, "hpmpc_mi355x_ocp_kkt_batch: plan")) return g_err;
    return hpmpc_mi355x_kkt_new_rhs_batch(O->tile.get(), nullptr, nprob, p0, count, 1, BAbt, RSQrq, DCt, nullptr,
                                          nullptr, d, ux, pi, lam, t, ws, scratch, 1, stream);
}

// A null direction is zero.
extern "C" int hpmpc_mi355x_kkt_tangent_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                              int p0, int count, int ndir, const double* BAbt, const double* RSQrq,
                                              const double* DCt, const double* db, const double* dq, const double* dd,
                                              double* dux, double* dpi, double* dlam, double* dt, const double* ws,
                                              double* scratch, int compute_mult, void* stream) {
    KArgs a;
    TanArgs x;
    memset(&x, 0, sizeof x);
    if (!sets_args(a, x.k, plan, lay, nprob, p0, count, ndir, BAbt, RSQrq, DCt, ws, scratch, dux && dpi && dlam && dt,
                   compute_mult, "hpmpc_mi355x_kkt_tangent_batch", "hpmpc_mi355x tangent call: ndir"))
        return g_err;
    set_arrays(a, db, dq, dd, dux, dpi, dlam, dt);
    if (const int e = hk_kkt_tan_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_tan launch failed");
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ocp_tangent_batch(const hpmpc_mi355x_ocp_plan* O, const hpmpc_mi355x_ocp_data* dirs,
                                              int nprob, int p0, int count, int ndir, const double* BAbt,
                                              const double* RSQrq, const double* DCt, double* du, double* dx,
                                              double* dpi, double* dlam, double* dt, const double* ws, double* scratch,
                                              int compute_mult, void* stream) {
    if (no_plan(O, "hpmpc_mi355x_ocp_tangent_batch: plan")) return g_err;
    KArgs a;
    TanArgs x;
    memset(&x, 0, sizeof x);
    const OcpOut out = ocp_out(O, du, dx, dpi, dlam, dt);
    if (!sets_args(a, x.k, O->tile.get(), nullptr, nprob, p0, count, ndir, BAbt, RSQrq, DCt, ws, scratch,
                   dirs && ocp_out_ok(out, true), compute_mult, "hpmpc_mi355x_ocp_tangent_batch",
                   "hpmpc_mi355x tangent call: ndir"))
        return g_err;
    for (int i = 0; i < OCP_NARR; i++) {
        const bool vec = ocp_is_vector(i);
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
    x.out = out;
    if (const int e = hk_kkt_tan_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_tan launch failed");
    return g_err = 0;
}

// A null cotangent is zero; a null bbar skips the multiplier half of the solve.
extern "C" int hpmpc_mi355x_kkt_adjoint_batch(const hpmpc_mi355x_plan* plan, const hpmpc_mi355x_layout* lay, int nprob,
                                              int p0, int count, int nadj, const double* BAbt, const double* RSQrq,
                                              const double* DCt, const double* gux, const double* gpi,
                                              const double* glam, const double* gt, double* bbar, double* qbar,
                                              double* dbar, const double* ws, double* scratch, void* stream) {
    KArgs a;
    AdjArgs x;
    memset(&x, 0, sizeof x);
    if (!sets_args(a, x.k, plan, lay, nprob, p0, count, nadj, BAbt, RSQrq, DCt, ws, scratch, qbar && dbar, bbar ? 1 : 0,
                   "hpmpc_mi355x_kkt_adjoint_batch", "hpmpc_mi355x adjoint call: nadj"))
        return g_err;
    set_arrays(a, gpi, gux, nullptr, qbar, bbar, dbar, nullptr);  // hk_adj_args.h: which KArgs field carries what
    x.glam = glam;
    x.gt = gt;
    if (const int e = hk_kkt_adj_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_adj launch failed");
    return g_err = 0;
}

namespace {

// The matrix entries of `grads` and the arrays they need -> m.  bbar / qbar / dbar and their strides are the caller's
// to set.  False: refused, g_err set.
bool matgrad_args(MatGradArgs& m, const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int nadj,
                  const double* ux, const double* pi, const double* lam, const hpmpc_mi355x_ocp_grads* grads,
                  const char* who) {
    memset(&m, 0, sizeof m);
    bool ab = false, cd = false;
    for (int i = 0; i < OCP_NARR; i++) {
        if (ocp_is_vector(i) || !grads->ptr[i]) continue;
        if (grads->stride[i] < O->dense[i]) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x matrix gradients: a stride below the array's size");
            return false;
        }
        if (O->dense[i] == 0) continue;  // a matrix the plan has no element of is never written
        m.grad.p[i] = grads->ptr[i];
        m.grad.s[i] = grads->stride[i];
        ab = ab || i == OCP_A || i == OCP_B;
        cd = cd || i == OCP_C || i == OCP_D;
    }
    if (!ux || (ab && !pi) || (cd && !lam)) {
        null_array(who);
        return false;
    }
    const long long n1 = O->N + 1;
    m.N = O->N;
    m.nprob = nprob;
    m.p0 = p0;
    m.count = count;
    m.nadj = nadj;
    m.row_major = O->row_major;
    m.st = O->d_st.get();
    m.ux = ux;
    m.pi = ab ? pi : nullptr;
    m.lam = cd ? lam : nullptr;
    m.sV16 = n1 * V16;
    m.sV32 = n1 * V32;
    return true;
}

bool wants_matrix(const hpmpc_mi355x_ocp_grads* g) {
    for (int i = 0; i < OCP_NARR; i++)
        if (!ocp_is_vector(i) && g->ptr[i]) return true;
    return false;
}

// hpmpc_mi355x_ocp_adjoint_batch and hpmpc_mi355x_ocp_adjoint_data_batch: the dense adjoint launch for the vector
// entries of `grads` and, when it has a matrix entry, the matrix gradients on the adjoint solution in the scratch, from
// the base iterate ux, pi, lam (not read otherwise, so they may be null).  The checks run range, arrays, stride, and
// every check of the second launch comes before the first.
int ocp_adjoint(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int nadj, const double* BAbt,
                const double* RSQrq, const double* DCt, const double* ux, const double* pi, const double* lam,
                const double* const cot[5], const hpmpc_mi355x_ocp_grads* grads, const double* ws, double* scratch,
                void* stream, const char* who) {
    KArgs a;
    AdjArgs x;
    memset(&x, 0, sizeof x);
    // any: the call has an output; mult: the multiplier half of the solve runs
    bool any = false, mult = false, bad_stride = false;
    for (int i = 0; grads && i < OCP_NARR; i++) {
        if (!grads->ptr[i]) continue;
        any = true;
        mult = mult || ((i == OCP_b || i == OCP_A || i == OCP_B) && O->dense[i] > 0);
        if (!ocp_is_vector(i)) continue;
        bad_stride = bad_stride || grads->stride[i] < O->dense[i];
        if (O->dense[i] > 0) {  // a vector the plan has no element of is never written
            x.grad.p[i] = grads->ptr[i];
            x.grad.s[i] = grads->stride[i];
        }
    }
    if (!sets_args(a, x.k, O->tile.get(), nullptr, nprob, p0, count, nadj, BAbt, RSQrq, DCt, ws, scratch, any, mult,
                   who, "hpmpc_mi355x adjoint call: nadj"))
        return g_err;
    if (bad_stride) {  // only the data call brings strides of its own
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_adjoint_data_batch: a stride below the array's size");
        return g_err;
    }
    const long long scot[5] = {O->su, O->sx, O->sp, O->sl, O->sl};
    for (int i = 0; i < 5; i++) {
        if (scot[i] > 0) {  // a cotangent the plan has no element of is never read
            x.cot[i].p = cot[i];
            x.cot[i].s = scot[i];
        }
    }
    x.ost = O->d_st.get();
    MatGradArgs m;
    const bool mats = wants_matrix(grads);
    if (mats) {
        if (!matgrad_args(m, O, nprob, p0, count, nadj, ux, pi, lam, grads, who)) return g_err;
        const KktSet c = carve_set(scratch, O->N);  // where hk_kkt_adj leaves the dense call's qbar, bbar, dbar
        m.qbar = c.dux;
        m.bbar = m.pi ? c.dpi : nullptr;
        m.dbar = m.lam ? c.res_d : nullptr;
        m.sq = m.sb = m.sd = x.k.sS;
    }
    if (const int e = hk_kkt_adj_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_adj launch failed");
    if (mats)
        if (const int e = hk_ocp_matgrad_launch(&m, (hipStream_t)stream))
            return launch_error(e, "hk_ocp_matgrad launch failed");
    return g_err = 0;
}

}  // namespace

extern "C" int hpmpc_mi355x_ocp_adjoint_batch(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int nadj,
                                              const double* BAbt, const double* RSQrq, const double* DCt,
                                              const double* gu, const double* gx, const double* gpi,
                                              const double* glam, const double* gt, double* gb, double* gq, double* gr,
                                              double* glb, double* gub, double* glg, double* gug, const double* ws,
                                              double* scratch, void* stream) {
    if (no_plan(O, "hpmpc_mi355x_ocp_adjoint_batch: plan")) return g_err;
    const double* cot[5] = {gu, gx, gpi, glam, gt};
    const struct {
        int i;
        double* p;
    } vec[] = {{OCP_b, gb}, {OCP_q, gq}, {OCP_r, gr}, {OCP_lb, glb}, {OCP_ub, gub}, {OCP_lg, glg}, {OCP_ug, gug}};
    hpmpc_mi355x_ocp_grads grads;
    memset(&grads, 0, sizeof grads);
    for (const auto& v : vec) {
        grads.ptr[v.i] = v.p;
        grads.stride[v.i] = O->dense[v.i];
    }
    return ocp_adjoint(O, nprob, p0, count, nadj, BAbt, RSQrq, DCt, nullptr, nullptr, nullptr, cot, &grads, ws, scratch,
                       stream, "hpmpc_mi355x_ocp_adjoint_batch");
}

extern "C" int hpmpc_mi355x_ocp_matrix_grads_batch(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count,
                                                   int nadj, const double* ux, const double* pi, const double* lam,
                                                   const double* bbar, const double* qbar, const double* dbar,
                                                   const hpmpc_mi355x_ocp_grads* grads, void* stream) {
    const char* who = "hpmpc_mi355x_ocp_matrix_grads_batch";
    if (no_plan(O, "hpmpc_mi355x_ocp_matrix_grads_batch: plan")) return g_err;
    g_err = 0;
    if (!range_ok(O, nprob, p0, count, who) || !sets_ok(nprob, nadj, "hpmpc_mi355x adjoint call: nadj") || count == 0)
        return g_err;
    if (!grads || !qbar) return null_array(who);
    for (int i = 0; i < OCP_NARR; i++) {
        if (ocp_is_vector(i) && grads->ptr[i]) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x_ocp_matrix_grads_batch: vector gradients (b, q, r, "
                                                    "lb, ub, lg, ug) are the adjoint call's");
            return g_err;
        }
    }
    if (!wants_matrix(grads)) return null_array(who);
    MatGradArgs m;
    if (!matgrad_args(m, O, nprob, p0, count, nadj, ux, pi, lam, grads, who)) return g_err;
    if ((m.pi && !bbar) || (m.lam && !dbar)) return null_array(who);
    m.qbar = qbar;
    m.bbar = m.pi ? bbar : nullptr;
    m.dbar = m.lam ? dbar : nullptr;
    m.sq = m.sb = m.sV16;
    m.sd = m.sV32;
    if (const int e = hk_ocp_matgrad_launch(&m, (hipStream_t)stream))
        return launch_error(e, "hk_ocp_matgrad launch failed");
    return g_err = 0;
}

namespace {

// The fourteen entries of `dirs` and the base iterate they need -> m.  db / dq / dd and their strides are the caller's
// to set.  False: refused, g_err set.
bool matdir_args(MatDirArgs& m, const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count, int ndir,
                 const double* ux, const double* pi, const double* lam, const hpmpc_mi355x_ocp_data* dirs,
                 const char* who) {
    memset(&m, 0, sizeof m);
    bool ab = false, cd = false;
    for (int i = 0; i < OCP_NARR; i++) {
        if (!dirs->ptr[i]) continue;
        if (dirs->stride[i] < O->dense[i]) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "hpmpc_mi355x matrix directions: a stride below the array's size");
            return false;
        }
        if (O->dense[i] == 0) continue;  // an array the plan has no element of is never read
        m.dir[i].p = dirs->ptr[i];
        m.dir[i].s = dirs->stride[i];
        ab = ab || i == OCP_A || i == OCP_B;
        cd = cd || i == OCP_C || i == OCP_D;
    }
    if (!ux || (ab && !pi) || (cd && !lam)) {
        null_array(who);
        return false;
    }
    const long long n1 = O->N + 1;
    m.N = O->N;
    m.nprob = nprob;
    m.p0 = p0;
    m.count = count;
    m.ndir = ndir;
    m.row_major = O->row_major;
    m.st = O->d_st.get();
    m.ux = ux;
    m.pi = ab ? pi : nullptr;
    m.lam = cd ? lam : nullptr;
    m.sV16 = n1 * V16;
    m.sV32 = n1 * V32;
    return true;
}

}  // namespace

extern "C" int hpmpc_mi355x_ocp_matrix_dirs_batch(const hpmpc_mi355x_ocp_plan* O, const hpmpc_mi355x_ocp_data* dirs,
                                                  int nprob, int p0, int count, int ndir, const double* ux,
                                                  const double* pi, const double* lam, double* db, double* dq,
                                                  double* dd, void* stream) {
    const char* who = "hpmpc_mi355x_ocp_matrix_dirs_batch";
    if (no_plan(O, "hpmpc_mi355x_ocp_matrix_dirs_batch: plan")) return g_err;
    g_err = 0;
    if (!range_ok(O, nprob, p0, count, who) || !sets_ok(nprob, ndir, "hpmpc_mi355x tangent call: ndir") || count == 0)
        return g_err;
    if (!dirs || !db || !dq || !dd) return null_array(who);
    MatDirArgs m;
    if (!matdir_args(m, O, nprob, p0, count, ndir, ux, pi, lam, dirs, who)) return g_err;
    m.db = db;
    m.dq = dq;
    m.dd = dd;
    m.sb = m.sq = m.sV16;
    m.sd = m.sV32;
    if (const int e = hk_ocp_matdir_launch(&m, (hipStream_t)stream))
        return launch_error(e, "hk_ocp_matdir launch failed");
    return g_err = 0;
}

// The seed launch into res_b / res_q / res_d of each set's scratch block, then hk_kkt_tan with its dense prologue
// skipped.  The checks run range, arrays, stride, and every check of the second launch comes before the first.
extern "C" int hpmpc_mi355x_ocp_tangent_data_batch(const hpmpc_mi355x_ocp_plan* O, const hpmpc_mi355x_ocp_data* dirs,
                                                   int nprob, int p0, int count, int ndir, const double* BAbt,
                                                   const double* RSQrq, const double* DCt, const double* ux,
                                                   const double* pi, const double* lam, double* du, double* dx,
                                                   double* dpi, double* dlam, double* dt, const double* ws,
                                                   double* scratch, int compute_mult, void* stream) {
    const char* who = "hpmpc_mi355x_ocp_tangent_data_batch";
    if (no_plan(O, "hpmpc_mi355x_ocp_tangent_data_batch: plan")) return g_err;
    KArgs a;
    TanArgs x;
    memset(&x, 0, sizeof x);
    const OcpOut out = ocp_out(O, du, dx, dpi, dlam, dt);
    if (!sets_args(a, x.k, O->tile.get(), nullptr, nprob, p0, count, ndir, BAbt, RSQrq, DCt, ws, scratch,
                   dirs && ocp_out_ok(out, true), compute_mult, who, "hpmpc_mi355x tangent call: ndir"))
        return g_err;
    MatDirArgs m;
    if (!matdir_args(m, O, nprob, p0, count, ndir, ux, pi, lam, dirs, who)) return g_err;
    const KktSet c = carve_set(scratch, O->N);  // where hk_kkt_tan's dense prologue leaves the seed rows
    m.db = c.res_b;
    m.dq = c.res_q;
    m.dd = c.res_d;
    m.sb = m.sq = m.sd = x.k.sS;
    x.ost = O->d_st.get();
    x.out = out;
    if (const int e = hk_ocp_matdir_launch(&m, (hipStream_t)stream))
        return launch_error(e, "hk_ocp_matdir launch failed");
    if (const int e = hk_kkt_tan_seeded_launch(&a, &x, count, (hipStream_t)stream))
        return launch_error(e, "hk_kkt_tan launch failed");
    return g_err = 0;
}

extern "C" int hpmpc_mi355x_ocp_adjoint_data_batch(const hpmpc_mi355x_ocp_plan* O, int nprob, int p0, int count,
                                                   int nadj, const double* BAbt, const double* RSQrq,
                                                   const double* DCt, const double* ux, const double* pi,
                                                   const double* lam, const double* gu, const double* gx,
                                                   const double* gpi, const double* glam, const double* gt,
                                                   const hpmpc_mi355x_ocp_grads* grads, const double* ws,
                                                   double* scratch, void* stream) {
    if (no_plan(O, "hpmpc_mi355x_ocp_adjoint_data_batch: plan")) return g_err;
    const double* cot[5] = {gu, gx, gpi, glam, gt};
    return ocp_adjoint(O, nprob, p0, count, nadj, BAbt, RSQrq, DCt, ux, pi, lam, cot, grads, ws, scratch, stream,
                       "hpmpc_mi355x_ocp_adjoint_data_batch");
}

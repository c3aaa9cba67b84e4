// hk_plan.h -- the tile path's plan, the device tables and call checks of its batched API and the one-problem staging
// carve, shared by the host files of that path: hpmpc_capi.cpp (plan, layout tables, batched API; defines the plan
// functions and call checks below), hpmpc_capi_queue.cpp (the problem queue), hpmpc_capi_dropin.cpp (reference-named
// hard-constraint entry points; defines the arena functions), hpmpc_capi_soft.cpp (soft-constraint IPM and residual;
// defines the soft refusals, layout and IPM setup), hpmpc_capi_soft_batch.cpp (the batched soft-constraint IPM) and
// hpmpc_capi_ocp_soft.cpp (the soft OCP front end; both through hk_soft_plan.h), hpmpc_capi_ocp.cpp (the batched OCP
// front end) and hpmpc_capi_kkt.cpp (the batched KKT re-solve and its tangent solve; through hk_ocp_plan.h).
#pragma once
#include <climits>
#include <mutex>
#include <vector>

#include "hk_host.h"
#include "hk_soft_args.h"
#include "hpmpc_kargs.h"

struct StageInfoH {  // mirror of hk::StageInfo
    int nu, nx, nb, ng, xo, nx1, nu1, xo1, sdB, sdR, oB, oR, oD, pnb, r0, oG;
};

// Plan: stage tables shared by every problem of a batch.
struct hpmpc_mi355x_plan {
    int N = 0;
    std::vector<int> nx, nu, nb, ng;
    std::vector<std::vector<int>> idxb;
    std::vector<StageInfoH> st;
    std::vector<signed char> tileslot, slotvar;
    std::vector<long long> offB, offR;  // packed default layout
    long long packB = 0, packR = 0;
    DevTable<StageInfoH> d_st;  // the stage table of the packed default layout
    DevTable<signed char> d_tileslot, d_slotvar;
    // one device stage table per caller layout (hpmpc_mi355x_layout: offsets and shared-block flags differ), uploaded
    // the first time a layout is used and never rewritten: a launch still running on another stream keeps reading its
    // own layout's offsets while the next call uses a different one
    struct LayoutTable {
        std::vector<StageInfoH> st;
        DevTable<StageInfoH> d;
    };
    // at most kMaxLayouts, guarded by ltabs_mu (calls on one plan from several threads); a cache: a const plan fills it
    mutable std::vector<LayoutTable> ltabs;
    mutable std::mutex ltabs_mu;
    int fixcls = 0;                             // compiled inner-stage class (kernel instance)
    int nbt = 0;                                // sum of nb + ng
    int ngt = 0;                                // sum of ng
    std::vector<long long> offG;                // DCt_k offsets (packed), per stage
    long long packG = 0;
};

// Per-problem workspace (device carve in hpmpc_kernels.hip): rounded to 256 B, so that every slot of a batch or queue
// starts on a cache-line boundary and its 16- / 32-double stage vectors stay line-aligned (the certificate's N+1
// doubles alone would shift each slot by 8 B per stage: +50 % on the element-wise update pass, measured)
inline long long ws_doubles(int N) {
    const long long n = (long long)(N + 1) * (FSTRIDE + 9 * V16 + 8 * V32 + 1) + 16;
    return (n + 31) / 32 * 32;
}

// hpmpc_capi.cpp
bool plan_supported(int N, const int* nx, const int* nu, const int* nb, const int* const* idxb, const int* ng,
                    const char** why);
// 16 ints per stage: out[16 k + l] = idxb[k][l] for l < nb[k]; the other entries of `out` are left as they are
void idxb_table(int N, const int* nb, const int* const* idxb, int* out);
// The checks every batched call with a problem range makes, each setting HPMPC_MI355X_EUNSUPPORTED with one stderr
// line.  range_ok: a plan, nprob > 0 and 0 <= p0, 0 <= count, p0 + count <= nprob (without int overflow);
// null_array returns the code.  launch_error maps a launcher's nonzero return: HK_LAUNCH_REFUSED to
// HPMPC_MI355X_EUNSUPPORTED, anything else to HPMPC_MI355X_EHIP, and returns the code.
bool range_ok(const void* plan, int nprob, int p0, int count, const char* who);
int null_array(const char* who);
int launch_error(int e, const char* what);
// n sets per problem (right-hand sides, directions): the grid is count * n workgroups and a set index is an int.
// False: g_err set, with the message `what`.
inline bool sets_ok(int nprob, int n, const char* what) {
    if (n >= 1 && (long long)nprob * n <= INT_MAX) return true;
    hk_set_error(HPMPC_MI355X_EUNSUPPORTED, what);
    return false;
}
// The argument block of a batched call: the plan's tables and strides, the layout (null: the packed default; a
// layout's first use uploads its stage table) and DCt.  A call that carries no DCt array refuses a plan with
// ng > 0 (DCT_NONE); one that does passes it on when the plan has general constraints (DCT_ARRAY).  False: g_err set.
enum DctPolicy { DCT_NONE, DCT_ARRAY };
bool batch_args(KArgs& a, const hpmpc_mi355x_plan* P, const hpmpc_mi355x_layout* lay, int nprob, int p0,
                DctPolicy policy, const double* DCt = nullptr);
int launch(int which, const KArgs* a, int count, hipStream_t s);  // hk_launch, or the ric2 variant's two-wave sv
// the IPM fields of `a` (plan tables and layout already set) and the launch `which`: shared by every batched IPM call
int ipm_run(KArgs& a, int count, const double* BAbt, const double* RSQrq, const double* d, double* ux, double* pi,
            double* lam, double* t, double* ws, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
            int compute_mult, int* kk, int* ret, double* stat, int which, void* stream);
// the calling thread's cached plan for these sizes (created on first use, replaced when the sizes change)
hpmpc_mi355x_plan* thread_plan(int N, const int* nx, const int* nu, const int* nb, int** idxb, const int* ng);

// hpmpc_capi_dropin.cpp: the staging arena carve (doubles) of one problem on the thread's device context (g_dev)
struct Arena {
    size_t BAbt, RSQ, DCt, d, ux, pi, lam, t, ws, vb, vq, vQx, vqx, vPb, stat, ints, qctl, total;
};
Arena arena(const hpmpc_mi355x_plan* P, int k_max);
KArgs arena_args(const hpmpc_mi355x_plan* P, const Arena& A, double* dev);
// copy stage blocks (lib4, possibly aliased) into the packed arena layout
void stage_BAbt(const hpmpc_mi355x_plan* P, double* H, const Arena& A, double** hpBAbt);
void stage_RSQ(const hpmpc_mi355x_plan* P, double* H, const Arena& A, double** hpQ);
bool run(int which, const KArgs& a, const char* name);  // one-problem launch on g_dev.stream
// Per-stage caller vectors <-> a strided arena region (V16 per stage; V32 for the constraint vectors).  Lengths:
// VEC_UX nu+nx, VEC_PI nx[k+1] (none at stage N), VEC_CV the constraint vector (none on a stage with nb + ng = 0);
// a stage whose length is 0 is skipped, so that caller buffer is neither read nor written.
enum VecKind { VEC_UX, VEC_PI, VEC_CV };
void vec_in(const hpmpc_mi355x_plan* P, VecKind kind, double* H, size_t off, double** v);
void vec_out(const hpmpc_mi355x_plan* P, VecKind kind, double** v, const double* H, size_t off);

// hpmpc_capi_soft.cpp: what the soft-constraint IPM refuses and how it lays out its vectors, for the reference-named
// entry point and the batched one alike.  Both return null, or the reason for HPMPC_MI355X_EUNSUPPORTED.
struct SoftLayout {
    std::vector<SoftStage> st;
    long sC = 0, sD = 0, sZ = 0;  // doubles per problem of t / lam, d, Z / z
    long sF = 0;                  // the flat Qx / qx | Zl / zl block with the reference's padding
};
// What d_ip2_mpc_soft_tv and the batched soft IPM set alike: 1 / sum(2 nb + 4 ns) (0: no constraint anywhere), the
// Riccati flags of their sv / trs steps, and the scalar fields of a zeroed SoftArgs
double soft_mu_scal(int N, const int* nb, const int* ns);
void soft_ric_flags(KArgs& a, int compute_mult);
SoftArgs soft_scalars(int N, int nprob, int p0, int k_max, int warm_start, double mu0, double mu_tol, double alpha_min,
                      double mu_scal);
// ng > 0, nu[N] != 0, N < 1, or a b_k the reference reads outside BAbt_k
const char* soft_unsupported(int N, const int* nx, const int* nu, const int* ng);
// the layout; refuses the stray soft-gradient write into a Zl its pass still reads
const char* soft_layout(int N, const int* nx, const int* nu, const int* nb, const int* ns, SoftLayout& L);

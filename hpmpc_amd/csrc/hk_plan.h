// hk_plan.h -- the tile path's plan and the one-problem staging carve, shared by the host files of that path:
// hpmpc_capi.cpp (plan, layout tables, batched API; defines the plan functions below), hpmpc_capi_queue.cpp (the
// problem queue), hpmpc_capi_dropin.cpp (reference-named hard-constraint entry points; defines the arena functions)
// hpmpc_capi_soft.cpp (soft-constraint IPM and residual; defines the soft refusals and layout),
// hpmpc_capi_soft_batch.cpp (the batched soft-constraint IPM) and hpmpc_capi_kkt.cpp (the batched KKT re-solve).
#pragma once
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
    void* d_st = nullptr;  // the stage table of the packed default layout (uploaded once, never rewritten)
    signed char *d_tileslot = nullptr, *d_slotvar = nullptr;
    // one device stage table per caller layout (hpmpc_mi355x_layout: offsets and shared-block flags differ), uploaded
    // the first time a layout is used and never rewritten: a launch still running on another stream keeps reading its
    // own layout's offsets while the next call uses a different one
    struct LayoutTable {
        std::vector<StageInfoH> st;
        void* d = nullptr;
    };
    std::vector<LayoutTable> ltabs;  // at most kMaxLayouts, guarded by ltabs_mu (calls on one plan from several threads)
    std::mutex ltabs_mu;
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
KArgs base_args(const hpmpc_mi355x_plan* P, int nprob, int p0);
bool layout_apply(hpmpc_mi355x_plan* P, const hpmpc_mi355x_layout* lay, KArgs& a);
// layout_apply without its ng > 0 refusal, for the calls that carry a DCt array (hpmpc_capi_kkt.cpp)
bool layout_set(hpmpc_mi355x_plan* P, const hpmpc_mi355x_layout* lay, KArgs& a);
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
// ng > 0, nu[N] != 0, N < 1, or a b_k the reference reads outside BAbt_k
const char* soft_unsupported(int N, const int* nx, const int* nu, const int* ng);
// the layout; refuses the stray soft-gradient write into a Zl its pass still reads
const char* soft_layout(int N, const int* nx, const int* nu, const int* nb, const int* ns, SoftLayout& L);

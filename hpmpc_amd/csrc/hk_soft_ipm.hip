// hk_soft_ipm.hip -- MI355X (gfx950): the whole soft-constraint IPM d_ip2_mpc_soft_tv (mpc_solvers/d_ip2_soft.c:83-547)
// of a problem in one launch, for device-resident batches (hpmpc_mi355x_ipm_soft_batch).
//
// One wavefront per problem, grid = problems; the soft counterpart of hk_ipm_solo (hpmpc_kernels.hip).  The wave
// runs its problem's loop
//     while active:  hess -> ric_backward + ric_forward_sv -> pred -> ric_trs -> corr
// with the constraint passes of hk_soft_body.h (the functions hk_soft_pass runs one per launch) and the Riccati
// bodies of hk_riccati.h called as hk_ric_sv / hk_ric_trs call them, and returns when its own exit test fires, so
// a problem that converges early frees its CU slot.  No host poll, no launch between the passes.  The bodies hand
// data to each other through global memory (one lane writes, another reads): a workgroup barrier separates them.
// hk_soft_ipm_init, its own launch right before, starts the solve (see there).
#include "hk_ipm_body.h"
#include "hk_launch.h"
#include "hk_soft_body.h"

namespace {

// The problem index behind an opaque wave-uniform value: every body re-derives its pointers from the kernel
// arguments, so nothing of one body stays live across the next (hk_ipm_solo's remedy against scratch spills).
__device__ __forceinline__ int opaque_prob(int p) {
    asm volatile("" : "+v"(p));
    return __builtin_amdgcn_readfirstlane(p);
}

}  // namespace

// Start of a batched solve: clears the problem's work arrays behind the factor (the caller's workspace arrives
// uninitialised, and the Riccati vectors are read over whole 16-slot stages), d_init_var_mpc_soft_tv with the
// loop-control state (soft_init), and the Riccati right-hand sides from the device arrays with the index
// arithmetic of the reference-named entry point: q_k = the augmented row of RSQrq_k, b_k = the augmented row of
// BAbt_k with the reference's panel stride round_up(nx_{k+1}, 4) (d_ip2_soft.c:172), each block found through
// the layout's stage table (per-stage offsets, shared-block flags).
__global__ __launch_bounds__(64) void hk_soft_ipm_init(KArgs a, SoftArgs s) {
    using namespace hk_soft;
    const int p = blockIdx.x + a.p0;
    if (p >= a.nprob) return;
    const int l = threadIdx.x & 63;
    double* W = a.ws + (long)p * a.sW;
    for (long i = (long)(a.N + 1) * FSTRIDE + l; i < a.sW; i += 64) W[i] = 0.0;
    __syncthreads();
    const Prob P = prob(s, p);
    soft_init(s, P);
    const hk::StageInfo* st = reinterpret_cast<const hk::StageInfo*>(a.st);
    double* vb = s.vb + (long)p * s.sW;
    double* vq = s.vq + (long)p * s.sW;
    for (int q = 0; q < s.nq; q++) {
        const Lane L = lane_at(s, q);
        if (!L.ok) continue;
        const hk::StageInfo si = st[L.k];
        const int nux = si.nu + si.nx;
        const long row = (long)(nux >> 2) * 4;  // the augmented row nux: panel nux / 4, line nux % 4
        if (L.c < nux) {
            const double* R = ((si.r0 & 4) ? a.RSQ : a.RSQ + (long)p * a.sR) + si.oR;
            vq[L.k * V16 + L.c] = R[row * si.sdR + (nux & 3) + 4 * L.c];
        }
        if (L.k < a.N && L.c < si.nx1) {
            const double* B = ((si.r0 & 2) ? a.BAbt : a.BAbt + (long)p * a.sB) + si.oB;
            vb[L.k * V16 + L.c] = B[row * ((si.nx1 + 3) & ~3) + (nux & 3) + 4 * L.c];
        }
    }
}

// KArgs: the tile plan's tables and data (BAbt, RSQ with the layout's strides), ws = the per-problem workspace
// (factor first), and ux / pi / vb / vq / vQx / vqx / vPb = the Riccati vectors inside that workspace (sV16 = sW);
// the flags of the reference-named entry point (use_box, update_q, compute_Pb for the sv; the trs reads P b).
// SoftArgs: the constraint data, the iterate and the work arrays of the passes.
template <class FX>
__global__ __launch_bounds__(64) void hk_soft_ipm(KArgs a, SoftArgs s) {
    using namespace hk_soft;
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int p = blockIdx.x + a.p0;
    if (p >= a.nprob) return;
    for (int it = 0; it < s.k_max; it++) {  // the exit test (ist[1]) ends the loop; k_max bounds it regardless
        wsync();
        {
            const Prob P = prob(s, opaque_prob(p));
            if (!P.ist[1]) break;
            soft_hess(s, P);
        }
        wsync();
        {
            const int q = opaque_prob(p);
            RicIO io = make_io(a, T, q, a.ws + (long)q * a.sW);
            const long o16 = (long)q * a.sV16;
            BoxCtx bc{};
            bc.Qx = a.vQx + o16;
            bc.qx = a.vqx + o16;
            ric_backward<true, BX_GIVEN, FX, CERT_LOAD>(io, &sm, a.update_b, a.vb + o16, a.update_q, a.vq + o16, bc,
                                                        a.compute_Pb, a.vPb + o16);
            wsync();
            ric_forward_sv<FX>(io, &sm, a.update_b, a.vb + o16, a.ux + o16, a.compute_pi, a.pi + o16);
        }
        wsync();
        {
            const Prob P = prob(s, opaque_prob(p));
            soft_pred(s, P, P.stat + 5 * P.ist[0]);
        }
        wsync();
        {
            const int q = opaque_prob(p);
            RicIO io = make_io(a, T, q, a.ws + (long)q * a.sW);
            const long o16 = (long)q * a.sV16;
            BoxCtx bc{};
            bc.qx = a.vqx + o16;
            double al = 1.0;
            ric_trs<BX_GIVEN, BX_NONE, FX>(io, &sm, a.vb + o16, a.vq + o16, bc, a.ux + o16, a.compute_pi, a.pi + o16, 0,
                                           a.vPb + o16, al);
        }
        wsync();
        {
            const Prob P = prob(s, opaque_prob(p));
            const int kk = P.ist[0];
            soft_corr(s, P, P.stat + 5 * kk, kk);
        }
    }
    wsync();
    if ((threadIdx.x & 63) == 0) {
        const Prob P = prob(s, p);
        s.kk[p] = P.ist[0];
        s.ret[p] = P.ist[2];
    }
}

template <class FX>
static int soft_ipm_launch_t(const KArgs* a, const SoftArgs* s, int count, hipStream_t stream) {
    // the launch guard (hk_launch_guard.h): LDS tables, private segment against the stack limit, launch bound
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_soft_ipm<FX>));
    const size_t lds = lds_table_bytes(a->N);
    if (const int e = lim.check(lds, 64)) return e;
    hipLaunchKernelGGL(hk_soft_ipm_init, dim3(count), dim3(64), 0, stream, *a, *s);
    hipLaunchKernelGGL(hk_soft_ipm<FX>, dim3(count), dim3(64), lds, stream, *a, *s);
    return (int)hipGetLastError();
}

// The compiled inner-stage class is the tile plan's (KArgs.fixcls), as in hk_launch.
extern "C" int hk_soft_ipm_launch(const KArgs* a, const SoftArgs* s, int count, hipStream_t stream) {
    if (count <= 0) return 0;
    return with_fixcls(a->fixcls, [&](auto fx) {
        return soft_ipm_launch_t<typename decltype(fx)::type>(a, s, count, stream);
    });
}

// hk_matgrad.hip -- MI355X (gfx950): the OCP matrix gradients (hpmpc_mi355x_ocp_matrix_grads_batch,
// hpmpc_mi355x_ocp_adjoint_data_batch).
//
// hk_ocp_matgrad: from the adjoint solution (bbar, qbar = [rbar | qxbar], dbar) of a cotangent set and the base iterate
// (ux = [u | x], pi, lam) of its problem, the gradients with respect to the dense matrices: per stage k
//   gA = bbar x' + pi qxbar'        gB = bbar u' + pi rbar'
//   gQ = (qxbar x' + x qxbar') / 2  gR = (rbar u' + u rbar') / 2    gS = rbar x' + u qxbar'
//   gC = w qxbar' - s x'            gD = w rbar' - s u'             w = lam_ug - lam_lg, s = dbar_lg + dbar_ug
// the transpose of the residuals' dependence on the matrices at a fixed iterate (include/hpmpc_mi355x.h).  The outer
// products of different stages and sets are independent, so this is a launch of its own, not an epilogue of the
// one-wavefront-per-set adjoint solve: one workgroup of one wavefront per (stage, set), stage fastest, so neighbouring
// workgroups store to neighbouring blocks of every array.  The stage's 128 input doubles go to LDS once; lane t then
// owns elements t, t + 64, .. of the wanted dense blocks of the stage laid end to end (the hk_ocp_pack pattern: a
// wavefront's stores are consecutive within a block), decodes (row, column) from the element index and the plan's
// storage order, and stores one value.  Every element of a wanted block is written exactly once, nothing else is; a
// block without elements (stage N's A, B, R, S, D; an empty x_0; a null output) takes no iteration.  Per set and stage
// nx1 (nu + nx) + (nu + nx)^2 + ng (nu + nx) doubles are written for at most 128 read: the kernel is store-bound.
// Workgroup size, measured at nprob 1024, N = 100, nx = 12, nu = 4 (448 doubles per stage and set), 4 sets per problem:
// 256 threads 0.83 ms, 128 threads 0.55 ms, 64 threads 0.43 ms.  A workgroup's fixed chain (stage table -> 128 loads ->
// LDS -> first store) is paid once per stage and set whatever its width, and a wavefront that owns the whole stage
// spreads it over seven store iterations where four wavefronts spread it over two each.
#include <hip/hip_runtime.h>

#include "hk_launch.h"
#include "hk_launch_guard.h"
#include "hk_matgrad_args.h"
#include "hk_ocp_place.h"

namespace {

constexpr int MG_THREADS = 64;
constexpr int MG_NMAT = 7;
// the stage's inputs in LDS: [ux | pi | qbar | bbar] V16 each, then [lam | dbar] V32 each
constexpr int MG_UX = 0, MG_PI = V16, MG_QBAR = 2 * V16, MG_BBAR = 3 * V16, MG_LAM = 4 * V16, MG_DBAR = 4 * V16 + V32;
constexpr int MG_ROW = 4 * V16 + 2 * V32;

// The symmetric outer product behind gR, gS and gQ, on the variable slots (vi, vj) of [u | x]: qbar_vi ux_vj + ux_vi
// qbar_vj, evaluated with the smaller slot first, so (vi, vj) and (vj, vi) give the same bits.
__device__ __forceinline__ double sym_outer(const double* qbar, const double* ux, int vi, int vj) {
    const int lo = vi < vj ? vi : vj, hi = vi < vj ? vj : vi;
    return qbar[lo] * ux[hi] + ux[lo] * qbar[hi];
}

}  // namespace

__global__ __launch_bounds__(MG_THREADS) void hk_ocp_matgrad(MatGradArgs a) {
    __shared__ double row[MG_ROW];
    const unsigned n1 = a.N + 1;
    const int k = blockIdx.x % n1;
    const unsigned j = blockIdx.x / n1;
    const unsigned pj = j / (unsigned)a.nadj;
    if (pj >= (unsigned)a.count) return;
    const long p = (long)a.p0 + pj;
    if (p >= a.nprob) return;
    const long s = p * a.nadj + j % (unsigned)a.nadj;
    const OcpStage st = a.st[k];
    const int tid = threadIdx.x;
    // the wanted blocks of the stage, end to end, in the arrays' order
    constexpr int key[MG_NMAT] = {OCP_A, OCP_B, OCP_Q, OCP_S, OCP_R, OCP_C, OCP_D};
    const int rows[MG_NMAT] = {st.nx1, st.nx1, st.nx, st.nu, st.nu, st.ng, st.ng};
    const int cols[MG_NMAT] = {st.nx, st.nu, st.nx, st.nx, st.nu, st.nx, st.nu};
    int cum[MG_NMAT + 1];
    double* outp[MG_NMAT];
    cum[0] = 0;
#pragma unroll
    for (int i = 0; i < MG_NMAT; i++) {
        double* g = a.grad.p[key[i]];
        cum[i + 1] = cum[i] + (g ? rows[i] * cols[i] : 0);
        outp[i] = g ? g + s * a.grad.s[key[i]] + st.dn[key[i]] : nullptr;
    }
    const int total = cum[MG_NMAT];
    if (total == 0) return;  // the whole workgroup
    for (int t = tid; t < MG_ROW; t += MG_THREADS) {
        const long o16 = p * a.sV16 + k * V16, o32 = p * a.sV32 + k * V32, e = t & 15, c = t & 31;
        const double* src;
        if (t < MG_PI)
            src = a.ux + o16 + e;
        else if (t < MG_QBAR)
            src = a.pi ? a.pi + o16 + e : nullptr;
        else if (t < MG_BBAR)
            src = a.qbar + s * a.sq + k * V16 + e;
        else if (t < MG_LAM)
            src = a.bbar ? a.bbar + s * a.sb + k * V16 + e : nullptr;
        else if (t < MG_DBAR)
            src = a.lam ? a.lam + o32 + c : nullptr;
        else
            src = a.dbar ? a.dbar + s * a.sd + k * V32 + c : nullptr;
        row[t] = src ? *src : 0.0;
    }
    __syncthreads();
    const double *ux = row + MG_UX, *pi = row + MG_PI, *qbar = row + MG_QBAR, *bbar = row + MG_BBAR;
    const double *lam = row + MG_LAM, *dbar = row + MG_DBAR;
    const bool rm = a.row_major != 0;
    for (int e = tid; e < total; e += MG_THREADS) {
        // the block of element e: the last one that starts at or before it (an empty block is passed over)
        int m = 0, base = 0, r = rows[0], c = cols[0];
        double* out = outp[0];
#pragma unroll
        for (int i = 1; i < MG_NMAT; i++) {
            if (e >= cum[i]) {
                m = i;
                base = cum[i];
                r = rows[i];
                c = cols[i];
                out = outp[i];
            }
        }
        const int l = e - base;
        int bi, bj;
        if (rm) {
            bi = l / c;
            bj = l - bi * c;
        } else {
            bj = l / r;
            bi = l - bj * r;
        }
        // the column's slot in [u | x]: a state for A, Q, S, C, an input for B, R, D
        const int vj = m == 1 || m == 4 || m == 6 ? ocp_slot_u(st, bj) : ocp_slot_x(st, bj);
        double v;
        if (m <= 1) {  // A, B
            v = bbar[bi] * ux[vj] + pi[bi] * qbar[vj];
        } else if (m <= 4) {  // Q, S, R: the row is a state for Q, an input for S and R
            const double g = sym_outer(qbar, ux, m == 2 ? ocp_slot_x(st, bi) : ocp_slot_u(st, bi), vj);
            v = m == 3 ? g : 0.5 * g;
        } else {  // C, D
            const int lo = ocp_slot_lg(st, bi), up = ocp_slot_ug(st, bi);
            v = (lam[up] - lam[lo]) * qbar[vj] - (dbar[lo] + dbar[up]) * ux[vj];
        }
        out[l] = v;
    }
}

extern "C" int hk_ocp_matgrad_launch(const MatGradArgs* a, hipStream_t stream) {
    if (a->count <= 0 || a->nadj <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_matgrad));
    if (const int e = lim.check(0, MG_THREADS)) return e;
    const long long blocks = (long long)a->count * a->nadj * (a->N + 1);
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    hipLaunchKernelGGL(hk_ocp_matgrad, dim3((unsigned)blocks), dim3(MG_THREADS), 0, stream, *a);
    return (int)hipGetLastError();
}

// hk_ocp.hip -- the batched OCP front end's kernels for gfx950: dense problem data (the c_interface.h wrappers' A,
// B, b, Q, S, R, q, r, lb, ub, C, D, lg, ug) -> lib4 stage blocks and padded bound vectors in the tile plan's
// packed layout (hk_ocp_pack; hk_ocp_pack_vectors for matrices = 0), and the solver's padded iterate -> the
// wrappers' outputs with the residual infinity norms (hk_ocp_finish).  All are pure data movement (hk_ocp_finish
// adds fabs / fmax only).
//
// hk_ocp_pack: one 256-thread workgroup per (section, stage, problem); the sections are the stage's BAbt_k block,
// its RSQrq_k block, and its DCt_k block with d_k (and ux_k).  A section reads only its own dense arrays (at most
// six pointers), taken from the argument block with the section as a run-time index, so the scalar registers hold
// one section's pointers and not all fourteen.  Thread t owns output doubles t, t + 256, .. of the block, so a
// wavefront stores 512 consecutive bytes; the element's (row, column) is decoded from its lib4 index and the value
// gathered from the stage's dense block (<= 2.5 KB, one or two cache lines per wavefront and matrix row).  Padding
// rows / columns and the unused part of the 32-double d slot are stored as zeros: every output element is written
// and the caller's buffers need no initialisation.
//
// hk_ocp_finish: one wavefront per problem walks the stages; lane l owns variable l of ux, row l of pi and
// compact constraint l of lam / t, and keeps the running maxima of |r_q|, |r_b|, |r_d| over exactly the elements
// outputs() of hpmpc_capi_iface.cpp visits; one butterfly reduction at the end.
#include <hip/hip_runtime.h>

#include "hk_launch.h"
#include "hk_launch_guard.h"
#include "hk_ocp_args.h"
#include "hpmpc_kargs.h"

namespace {

constexpr int PACK_THREADS = 256;

// (row, column) of element e of a lib4 matrix with panel stride sd
__device__ __forceinline__ void lib4_rc(int e, int sd, int& i, int& j) {
    const int pw = 4 * sd, panel = e / pw, rem = e - panel * pw;
    i = 4 * panel + (rem & 3);
    j = rem >> 2;
}
__device__ __forceinline__ int lib4_at(int sd, int i, int j) { return (i >> 2) * 4 * sd + (i & 3) + 4 * j; }

// element (i, j) of a dense m x n block with leading sizes (m, n): column-major, or row-major
__device__ __forceinline__ double dense(const double* M, bool rm, int m, int n, int i, int j) {
    return M[rm ? i * n + j : i + j * m];
}

// BAbt_k = [B'; A'; b'], (nu + nx + 1) x nx1
__device__ __forceinline__ double babt_elem(const OcpStage& s, const double* A, const double* B, const double* b,
                                            bool rm, int i, int j) {
    if (j >= s.nx1) return 0.0;
    if (i < s.nu) return dense(B, rm, s.nx1, s.nu, j, i);
    const int ix = i - s.nu;
    if (ix < s.nx) return dense(A, rm, s.nx1, s.nx, j, ix);
    return ix == s.nx ? b[j] : 0.0;
}

// RSQrq_k = [[R S]; [S' Q]; [r' q']], (nu + nx + 1) x (nu + nx), both triangles
__device__ __forceinline__ double rsq_elem(const OcpStage& s, const double* Q, const double* S, const double* R,
                                           const double* q, const double* r, bool rm, int i, int j) {
    const int nu = s.nu, nux = s.nu + s.nx;
    if (j >= nux || i > nux) return 0.0;
    if (i == nux) return j < nu ? r[j] : q[j - nu];
    if (i < nu) return j < nu ? dense(R, rm, nu, nu, i, j) : dense(S, rm, nu, s.nx, i, j - nu);
    return j < nu ? dense(S, rm, nu, s.nx, j, i - nu) : dense(Q, rm, s.nx, s.nx, i - nu, j - nu);
}

// DCt_k = [D'; C'], (nu + nx) x ng
__device__ __forceinline__ double dct_elem(const OcpStage& s, const double* C, const double* D, bool rm, int i, int j) {
    if (j >= s.ng || i >= s.nu + s.nx) return 0.0;
    return i < s.nu ? dense(D, rm, s.ng, s.nu, j, i) : dense(C, rm, s.ng, s.nx, j, i - s.nu);
}

// d_k = [lb pnb | ub pnb | lg png | ug png | 0 ..], 32 doubles
__device__ __forceinline__ double d_elem(const OcpStage& s, const double* lb, const double* ub, const double* lg,
                                         const double* ug, int e) {
    if (e < s.pnb) return e < s.nb ? lb[e] : 0.0;
    e -= s.pnb;
    if (e < s.pnb) return e < s.nb ? ub[e] : 0.0;
    e -= s.pnb;
    if (e < s.png) return e < s.ng ? lg[e] : 0.0;
    e -= s.png;
    return e < s.ng ? ug[e] : 0.0;
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

}  // namespace

__global__ __launch_bounds__(PACK_THREADS) void hk_ocp_pack(OcpPackArgs a) {
    const unsigned n1 = a.N + 1;
    const int sec = blockIdx.x % OCP_NSEC;
    const unsigned sp = blockIdx.x / OCP_NSEC;
    const int k = sp % n1;
    const unsigned pi = sp / n1;
    if (pi >= (unsigned)a.count) return;
    const long p = (long)a.p0 + pi;
    if (p >= a.nprob) return;
    const OcpStage* sg = a.st + k;  // run-time indices go to the table itself, so the copy below stays in registers
    const OcpStage s = *sg;
    const bool rm = a.row_major != 0;
    const int tid = threadIdx.x;
    // the section's dense arrays are neighbours in HkOcpArray: A B b | Q S R q r | lb ub C D lg ug
    const int first = sec == OCP_SEC_BABT ? OCP_A : sec == OCP_SEC_RSQ ? OCP_Q : OCP_lb;
    const int cnt = sec == OCP_SEC_BABT ? 3 : sec == OCP_SEC_RSQ ? 5 : 6;
    const double* P[6];
#pragma unroll
    for (int i = 0; i < 6; i++) {
        const int ai = first + (i < cnt ? i : 0);
        P[i] = a.in[ai].p + p * a.in[ai].s + sg->dn[ai];
    }
    const int nux = s.nu + s.nx, n = sg->n[sec], sd = sg->sd[sec];  // n = 0: the stage has no such block
    double* out = a.out[sec] + p * a.sout[sec] + sg->o[sec];
    for (int e = tid; e < n; e += PACK_THREADS) {
        int i, j;
        lib4_rc(e, sd, i, j);
        double v;
        if (sec == OCP_SEC_BABT)
            v = babt_elem(s, P[0], P[1], P[2], rm, i, j);
        else if (sec == OCP_SEC_RSQ)
            v = rsq_elem(s, P[0], P[1], P[2], P[3], P[4], rm, i, j);
        else
            v = dct_elem(s, P[2], P[3], rm, i, j);
        out[e] = v;
    }
    if (sec != OCP_SEC_DCT) return;
    if (tid >= 64 && tid < 64 + V32)
        a.d[p * a.sV32 + k * V32 + (tid - 64)] = d_elem(s, P[0], P[1], P[4], P[5], tid - 64);
    if (a.ux && tid >= 128 && tid < 128 + V16) {
        const int e = tid - 128;
        double v = 0.0;
        if (e < s.nu)
            v = a.u0[p * a.su + s.dn[OCP_r] + e];
        else if (e < nux)
            v = a.x0[p * a.sx + s.dn[OCP_q] + (e - s.nu)];
        a.ux[p * a.sV16 + k * V16 + e] = v;
    }
}

// matrices = 0: the vector parts alone -- the b row of BAbt_k, the r / q row of RSQrq_k, d_k (and ux_k); every other
// element stays as it was.  One wavefront per (stage, problem), four stages per workgroup: lanes 0..15 the b row,
// 16..31 the r / q row, 32..63 the 32 doubles of d_k.  (The three-section grid of hk_ocp_pack would launch 300 k
// workgroups with 16 to 32 busy threads each here.)
__global__ __launch_bounds__(PACK_THREADS) void hk_ocp_pack_vectors(OcpPackArgs a) {
    const unsigned groups = (a.N + 4) / 4;
    const unsigned pi = blockIdx.x / groups;
    const int k = (blockIdx.x % groups) * 4 + (threadIdx.x >> 6);
    if (pi >= (unsigned)a.count || k > a.N) return;
    const long p = (long)a.p0 + pi;
    if (p >= a.nprob) return;
    const OcpStage& s = a.st[k];
    const int l = threadIdx.x & 63, nu = s.nu, nux = s.nu + s.nx;
    const auto in = [&](int i) { return a.in[i].p + p * a.in[i].s + s.dn[i]; };
    if (l < 16) {
        if (s.n[OCP_SEC_BABT] > 0 && l < s.nx1)
            a.out[OCP_SEC_BABT][p * a.sout[OCP_SEC_BABT] + s.o[OCP_SEC_BABT] + lib4_at(s.sd[OCP_SEC_BABT], nux, l)] =
                in(OCP_b)[l];
    } else if (l < 32) {
        const int j = l - 16;
        if (j < nux)
            a.out[OCP_SEC_RSQ][p * a.sout[OCP_SEC_RSQ] + s.o[OCP_SEC_RSQ] + lib4_at(s.sd[OCP_SEC_RSQ], nux, j)] =
                j < nu ? in(OCP_r)[j] : in(OCP_q)[j - nu];
    } else {
        a.d[p * a.sV32 + k * V32 + (l - 32)] = d_elem(s, in(OCP_lb), in(OCP_ub), in(OCP_lg), in(OCP_ug), l - 32);
    }
    if (a.ux && l < V16) {
        double v = 0.0;
        if (l < nu)
            v = a.u0[p * a.su + s.dn[OCP_r] + l];
        else if (l < nux)
            v = a.x0[p * a.sx + s.dn[OCP_q] + (l - nu)];
        a.ux[p * a.sV16 + k * V16 + l] = v;
    }
}

__global__ __launch_bounds__(64) void hk_ocp_finish(OcpFinishArgs a) {
    if (blockIdx.x >= (unsigned)a.count) return;
    const long p = (long)a.p0 + blockIdx.x;
    if (p >= a.nprob) return;
    const int l = threadIdx.x;
    const double* d = a.d + p * a.sV32;
    const double* ux = a.ux + p * a.sV16;
    const double* pi = a.pi + p * a.sV16;
    const double* lam = a.lam + p * a.sV32;
    const double* t = a.t + p * a.sV32;
    const long n1 = a.N + 1;
    const double* rq = a.res + p * a.sRes;
    const double* rb = rq + n1 * V16;
    const double* rd = rb + n1 * V16;
    double* u = a.u + p * a.su;
    double* x = a.x + p * a.sx;
    double* po = a.po + p * a.sp;
    double* lamo = a.lamo + p * a.sl;
    double* to = a.to ? a.to + p * a.sl : nullptr;
    double mq = 0.0, mb = 0.0, md = 0.0;
    for (int k = 0; k <= a.N; k++) {
        const OcpStage s = a.st[k];
        const int nux = s.nu + s.nx;
        if (l < nux) {
            double v = ux[k * V16 + l];
            if (l < s.nu) {
                // the equality-box fix over the leading input boxes: u[idxb[j]] = lb[j] where lb[j] == ub[j]
                for (int j = 0; j < s.nbu; j++) {
                    const double lo = d[k * V32 + j], up = d[k * V32 + s.pnb + j];
                    if (a.idxb[k * 16 + j] == l && lo == up) v = lo;
                }
                u[s.dn[OCP_r] + l] = v;
            } else {
                x[s.dn[OCP_q] + (l - s.nu)] = v;
            }
            mq = fmax(mq, fabs(rq[k * V16 + l]));
        }
        if (l < s.nx1) {
            po[s.dn[OCP_b] + l] = pi[k * V16 + l];
            mb = fmax(mb, fabs(rb[k * V16 + l]));
        }
        if (l < 2 * s.nb + 2 * s.ng) {  // compact [lb nb | ub nb | lg ng | ug ng] from the padded slot
            int src;
            if (l < s.nb)
                src = l;
            else if (l < 2 * s.nb)
                src = s.pnb + (l - s.nb);
            else if (l < 2 * s.nb + s.ng)
                src = 2 * s.pnb + (l - 2 * s.nb);
            else
                src = 2 * s.pnb + s.png + (l - 2 * s.nb - s.ng);
            const int o = 2 * s.dn[OCP_lb] + 2 * s.dn[OCP_lg] + l;
            lamo[o] = lam[k * V32 + src];
            if (to) to[o] = t[k * V32 + src];
            md = fmax(md, fabs(rd[k * V32 + src]));
        }
    }
    mq = wave_max(mq);
    mb = wave_max(mb);
    md = wave_max(md);
    if (l == 0) {
        double* inf = a.inf + 4 * p;
        inf[0] = mq;
        inf[1] = mb;
        inf[2] = md;
        inf[3] = a.mu[p];
    }
}

extern "C" int hk_ocp_pack_launch(const OcpPackArgs* a, hipStream_t stream) {
    if (a->count <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_pack));
    static const HkKernelLimits lim_vec(reinterpret_cast<const void*>(&hk_ocp_pack_vectors));
    if (const int e = (a->matrices ? lim : lim_vec).check(0, PACK_THREADS)) return e;
    const long long blocks = (long long)a->count * (a->matrices ? (a->N + 1) * OCP_NSEC : (a->N + 4) / 4);
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    if (a->matrices)
        hipLaunchKernelGGL(hk_ocp_pack, dim3((unsigned)blocks), dim3(PACK_THREADS), 0, stream, *a);
    else
        hipLaunchKernelGGL(hk_ocp_pack_vectors, dim3((unsigned)blocks), dim3(PACK_THREADS), 0, stream, *a);
    return (int)hipGetLastError();
}

extern "C" int hk_ocp_finish_launch(const OcpFinishArgs* a, hipStream_t stream) {
    if (a->count <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_finish));
    if (const int e = lim.check(0, 64)) return e;
    hipLaunchKernelGGL(hk_ocp_finish, dim3(a->count), dim3(64), 0, stream, *a);
    return (int)hipGetLastError();
}

// hk_ocp.hip -- the batched OCP front end's kernels for gfx950: dense problem data (the c_interface.h wrappers' A,
// B, b, Q, S, R, q, r, lb, ub, C, D, lg, ug) -> lib4 stage blocks and padded bound vectors in the tile plan's
// packed layout (hk_ocp_pack; hk_ocp_pack_vectors for matrices = 0), and the solver's padded iterate -> the
// wrappers' outputs (hk_ocp_unpack: with the residual infinity norms for the finish, without them for the sets of a
// multi-set re-solve).  All are pure data movement (the finish adds fabs / fmax only); the vector placements are
// those of hk_ocp_place.h.
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
// hk_ocp_unpack: one wavefront per set (the finish: per problem) walks the stages; lane l owns variable l of ux, row
// l of pi and compact constraint l of lam / t, and for the finish keeps the running maxima of |r_q|, |r_b|, |r_d|
// over exactly the elements outputs() of hpmpc_capi_iface.cpp visits; one butterfly reduction at the end.
#include <hip/hip_runtime.h>

#include "hk_launch.h"
#include "hk_launch_guard.h"
#include "hk_ocp_elem.h"
#include "hk_ocp_place.h"

namespace {

constexpr int PACK_THREADS = 256;

// DCt_k = [D'; C'], (nu + nx) x ng (lib4_rc, dense, babt_elem, rsq_elem, wave_max: hk_ocp_elem.h)
__device__ __forceinline__ double dct_elem(const OcpStage& s, const double* C, const double* D, bool rm, int i, int j) {
    if (j >= s.ng || i >= s.nu + s.nx) return 0.0;
    return i < s.nu ? dense(D, rm, s.ng, s.nu, j, i) : dense(C, rm, s.ng, s.nx, j, i - s.nu);
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
    const int n = sg->n[sec], sd = sg->sd[sec];  // n = 0: the stage has no such block
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
    if (tid >= 64 && tid < 64 + V32) {
        const auto in = [&](int i) { return a.in[i].p + p * a.in[i].s; };
        const OcpVecs v{nullptr, nullptr, nullptr, in(OCP_lb), in(OCP_ub), in(OCP_lg), in(OCP_ug)};
        a.d[p * a.sV32 + k * V32 + (tid - 64)] = __longlong_as_double(ocp_d_bits(s, v, tid - 64));
    }
    if (a.ux && tid >= 128 && tid < 128 + V16)
        a.ux[p * a.sV16 + k * V16 + (tid - 128)] = ocp_warm_elem(s, a.u0 + p * a.su, a.x0 + p * a.sx, tid - 128);
}

// matrices = 0: the vector parts alone -- the b row of BAbt_k, the r / q row of RSQrq_k, d_k (and ux_k); every other
// element stays as it was.  One wavefront per (stage, problem), four stages per workgroup; lane l stores element l
// of the stage's seed row (hk_ocp_place.h): lanes 0..15 the b row, 16..31 the r / q row, 32..63 the 32 doubles of
// d_k.  (The three-section grid of hk_ocp_pack would launch 300 k workgroups with 16 to 32 busy threads each here.)
__global__ __launch_bounds__(PACK_THREADS) void hk_ocp_pack_vectors(OcpPackArgs a) {
    const unsigned groups = (a.N + 4) / 4;
    const unsigned pi = blockIdx.x / groups;
    // the wavefront's stage, as a scalar: the seed row's loads take wave-uniform bases
    const int k = (blockIdx.x % groups) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (pi >= (unsigned)a.count || k > a.N) return;
    const long p = (long)a.p0 + pi;
    if (p >= a.nprob) return;
    const OcpStage& s = a.st[k];
    const int l = threadIdx.x & 63, nux = s.nu + s.nx;
    const auto in = [&](int i) { return a.in[i].p + p * a.in[i].s; };
    const OcpVecs v{in(OCP_b), in(OCP_q), in(OCP_r), in(OCP_lb), in(OCP_ub), in(OCP_lg), in(OCP_ug)};
    const double val = __longlong_as_double(ocp_seed_bits(s, v, l));
    if (l < 16) {
        if (s.n[OCP_SEC_BABT] > 0 && l < s.nx1)
            a.out[OCP_SEC_BABT][p * a.sout[OCP_SEC_BABT] + s.o[OCP_SEC_BABT] + lib4_at(s.sd[OCP_SEC_BABT], nux, l)] = val;
    } else if (l < 32) {
        if (l - 16 < nux)
            a.out[OCP_SEC_RSQ][p * a.sout[OCP_SEC_RSQ] + s.o[OCP_SEC_RSQ] + lib4_at(s.sd[OCP_SEC_RSQ], nux, l - 16)] = val;
    } else {
        a.d[p * a.sV32 + k * V32 + (l - 32)] = val;
    }
    if (a.ux && l < V16) a.ux[p * a.sV16 + k * V16 + l] = ocp_warm_elem(s, a.u0 + p * a.su, a.x0 + p * a.sx, l);
}

// RES: the finish -- one set per problem (the host's guarantee), and the residual maxima and mu go to a.inf.
template <bool RES>
__global__ __launch_bounds__(64) void hk_ocp_unpack(OcpUnpackArgs a) {
    const unsigned nsets = RES ? 1u : (unsigned)a.nsets;
    const unsigned pi_ = blockIdx.x / nsets;
    const long p = (long)a.p0 + pi_;
    if (pi_ >= (unsigned)a.count || p >= a.nprob) return;
    const long s = p * nsets + blockIdx.x % nsets;
    const int l = threadIdx.x;
    const double* d = a.d + s * a.sV32;
    const double* ux = a.ux + s * a.sV16;
    const double* pi = a.pi + s * a.sV16;
    const double* lam = a.lam + s * a.sV32;
    const double* t = a.t + s * a.sV32;
    const double *rq = nullptr, *rb = nullptr, *rd = nullptr;
    if constexpr (RES) {
        rq = a.res + p * a.sRes;
        rb = rq + (a.N + 1) * V16;
        rd = rb + (a.N + 1) * V16;
    }
    const OcpOut o = ocp_out_at(a.out, s);
    double mq = 0.0, mb = 0.0, md = 0.0;
    for (int k = 0; k <= a.N; k++) {
        const OcpStage os = a.st[k];
        const bool hv = l < os.nu + os.nx, hp = l < os.nx1, hc = l < 2 * os.nb + 2 * os.ng;
        const int src = k * V32 + compact_src(os, hc ? l : 0);
        ocp_unpack_store(os, o, l, hv ? ux[k * V16 + l] : 0.0, hp ? pi[k * V16 + l] : 0.0, hc ? lam[src] : 0.0,
                         hc && o.t ? t[src] : 0.0, d + k * V32, a.idxb + k * 16);
        if constexpr (RES) {
            if (hv) mq = fmax(mq, fabs(rq[k * V16 + l]));
            if (hp) mb = fmax(mb, fabs(rb[k * V16 + l]));
            if (hc) md = fmax(md, fabs(rd[src]));
        }
    }
    if constexpr (RES) {
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

// a->res set: the finish (residual maxima; one set per problem), else the plain unpack of count * nsets sets
extern "C" int hk_ocp_unpack_launch(const OcpUnpackArgs* a, hipStream_t stream) {
    if (a->count <= 0 || a->nsets <= 0) return 0;
    if (a->res && a->nsets != 1) return HK_LAUNCH_REFUSED;
    const auto kernel = a->res ? &hk_ocp_unpack<true> : &hk_ocp_unpack<false>;
    static const HkKernelLimits lim[2] = {HkKernelLimits(reinterpret_cast<const void*>(&hk_ocp_unpack<false>)),
                                          HkKernelLimits(reinterpret_cast<const void*>(&hk_ocp_unpack<true>))};
    if (const int e = lim[a->res ? 1 : 0].check(0, 64)) return e;
    const long long blocks = (long long)a->count * a->nsets;
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    hipLaunchKernelGGL(kernel, dim3((unsigned)blocks), dim3(64), 0, stream, *a);
    return (int)hipGetLastError();
}

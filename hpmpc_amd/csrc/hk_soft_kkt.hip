// hk_soft_kkt.hip -- MI355X (gfx950): the batched KKT re-solve for soft-constrained batches, many right-hand-side sets
// per factor (hpmpc_mi355x_soft_kkt_batch, hpmpc_mi355x_soft_kkt_ocp_batch).  The reference has no
// d_kkt_solve_new_rhs_* for its soft IPM: the call is an extension, defined in include/hpmpc_mi355x.h and DESIGN.md §3d.
//
// A linearisation is (Lam, tau) in the layout of lam -- Lam = lam / t at some iterate, tau its t -- with Zl and the
// Riccati factor of RSQrq_k + diag(Qx_k) built from Lam and Z as soft_hess (hk_soft_body.h) builds them.  For one set
// (b, q, d, z) the result is the affine (sigma mu = 0) Newton point: t' from the constraint rows, lam' = Lam (tau - t'),
// the slacks from their stationarity rows, ux' and pi' from one Riccati solve.
//
// hk_soft_kkt_factor: one wavefront per problem, grid = problems.  Writes tinv, lamt, Qx (flat block and the Riccati's
// V16 slots) and Zl into the problem's workspace from a given (lam, t), then factorises (ric_backward, BX_GIVEN, as
// hk_ric_trf calls it).  hk_soft_kkt_rhs: one wavefront per (problem, set), grid = count * nrhs, set s = p * nrhs + r.
// It reads Lam = lamt, tau = 1 / tinv and Zl from the workspace (not zl, the flat qx, vqx or Pb, which the IPM's
// corrector has changed), forms the box gradient in the set's scratch, runs ric_trs with a fresh P b and writes the
// set's ux, pi, lam, t.  The workspace is read only there, so any number of re-solves may follow one solve or one
// factor launch.  The conventions are hk_soft_ipm's: lane 16 g + c owns slot c of stage 4 q + g, a workgroup barrier
// between bodies that exchange data through global memory, pointers re-derived per body behind opaque_prob.
//
// hk_ocp_soft_kkt_pack: the dense per-set vectors b, q, r, lb, ub (z) of the soft OCP front end -> the sets' padded
// vectors, one wavefront per (stage, set), four stages per workgroup, with hk_ocp_soft_pack_vec's placement (the b /
// [r | q] rows through hk_ocp_place.h).  The sets are unpacked by hk_ocp_soft_unpack with a set in a problem's place.
#include "hk_ipm_body.h"
#include "hk_launch.h"
#include "hk_launch_guard.h"
#include "hk_ocp_place.h"
#include "hk_soft_kkt_args.h"

namespace {

__device__ __forceinline__ int opaque_prob(int p) {
    asm volatile("" : "+v"(p));
    return __builtin_amdgcn_readfirstlane(p);
}

struct KLane {
    int k, c;
    bool ok;
};
__device__ __forceinline__ KLane klane_at(int N, int q) {
    const int l = threadIdx.x & 63;
    KLane L;
    L.k = 4 * q + (l >> 4);
    L.c = l & 15;
    L.ok = L.k <= N;
    return L;
}

// The linearisation inside problem p's workspace
struct Lin {
    double *lamt, *tinv, *flat, *vQx;
};
__device__ __forceinline__ Lin lin_of(const KArgs& a, const SoftKktArgs& x, int p) {
    double* W = a.ws + (long)p * a.sW;
    return {W + x.oLamt, W + x.oTinv, W + x.oFlat, W + x.oVQx};
}

// soft_hess's tinv, lamt, Qx and Zl at (lam, t): the parts of d_update_hessian_mpc_soft_tv that depend on neither d
// nor z, with its arithmetic
__device__ inline void kkt_lin(const KArgs& a, const SoftKktArgs& x, int p) {
    const Lin W = lin_of(a, x, p);
    const double* lam = x.lam0 + (long)p * x.sC;
    const double* t = x.t0 + (long)p * x.sC;
    const double* Zp = x.Z + (long)p * x.sZ;
    for (int q = 0; q < x.nq; q++) {
        const KLane L = klane_at(a.N, q);
        if (!L.ok) continue;
        const SoftStage s = x.st[L.k];
        double* Qx = W.flat + s.oQ;
        if (L.c < s.nb) {
            const int lo = s.oC + L.c, up = lo + s.pnb;
            const double til = 1.0 / t[lo], tiu = 1.0 / t[up];
            const double ltl = lam[lo] * til, ltu = lam[up] * tiu;
            W.tinv[lo] = til;
            W.tinv[up] = tiu;
            W.lamt[lo] = ltl;
            W.lamt[up] = ltu;
            const double Q = ltl + ltu;
            Qx[L.c] = Q;
            W.vQx[L.k * V16 + L.c] = Q;
        } else if (L.c < s.nb + s.ns) {
            const int i = L.c - s.nb, pns = s.pns, b0 = s.oC + 2 * s.pnb + i;
            double lt[4];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int e = b0 + j * pns;
                const double ti = 1.0 / t[e];
                W.tinv[e] = ti;
                lt[j] = lam[e] * ti;
                W.lamt[e] = lt[j];
            }
            const double* Z = Zp + s.oZ;
            double rQx0 = lt[0], rQx1 = lt[1];
            double* Zl = W.flat + s.oZl;
            const double Zl0 = 1.0 / (Z[i] + rQx0 + lt[2]);
            const double Zl1 = 1.0 / (Z[pns + i] + rQx1 + lt[3]);
            Zl[i] = Zl0;
            Zl[pns + i] = Zl1;
            rQx0 = rQx0 - rQx0 * rQx0 * Zl0;
            rQx1 = rQx1 - rQx1 * rQx1 * Zl1;
            const double Q = rQx1 + rQx0;
            Qx[L.c] = Q;
            W.vQx[L.k * V16 + L.c] = Q;
        }
    }
}

// One set's vectors and its problem's linearisation
struct SetView {
    const double *lamt, *tinv, *flat, *d, *z;
    double *lam, *t, *ux, *qx;
};
__device__ __forceinline__ SetView set_view(const KArgs& a, const SoftKktArgs& x, int p, int r) {
    const long s = (long)p * x.nrhs + r;
    const Lin W = lin_of(a, x, p);
    SetView v;
    v.lamt = W.lamt;
    v.tinv = W.tinv;
    v.flat = W.flat;
    v.d = x.d + s * x.sDs;
    v.z = x.z ? x.z + s * x.sZs : x.z0 + (long)p * x.sZ;
    v.lam = x.lam + s * x.sCs;
    v.t = x.t + s * x.sCs;
    v.ux = a.ux + s * a.sV16;
    v.qx = x.scratch + s * x.sS;
    return v;
}

// A soft box's part of the linearisation and of the set's data: Lam and Lam tau of its four rows, Zl, and zl as
// soft_hess forms it with lam replaced by Lam tau
struct SoftBox {
    double lt[4], tau[4], Zl0, Zl1, zl0, zl1, rqx0, rqx1;
};
__device__ __forceinline__ SoftBox soft_box(const SetView& v, const SoftStage& s, int i) {
    const int pns = s.pns, b0 = s.oC + 2 * s.pnb + i;
    SoftBox B;
    double la[4];
#pragma unroll
    for (int j = 0; j < 4; j++) {
        const int e = b0 + j * pns;
        B.lt[j] = v.lamt[e];
        B.tau[j] = 1.0 / v.tinv[e];
        la[j] = B.lt[j] * B.tau[j];
    }
    const double* Zl = v.flat + s.oZl;
    const double* zz = v.z + s.oZ;
    const double dls = v.d[s.oD + 2 * s.pnb + i], dus = v.d[s.oD + 2 * s.pnb + pns + i];
    B.Zl0 = Zl[i];
    B.Zl1 = Zl[pns + i];
    B.rqx0 = la[0] + B.lt[0] * dls;
    B.rqx1 = la[1] - B.lt[1] * dus;
    B.zl0 = -zz[i] + B.rqx0 + la[2];
    B.zl1 = -zz[pns + i] + B.rqx1 + la[3];
    return B;
}

// The box gradient of the set in the Riccati's qx slots: the algebra of soft_hess's g and zl with lam = Lam tau.  A
// soft box's term goes to its own slot
__device__ inline void kkt_gradient(const KArgs& a, const SoftKktArgs& x, const SetView& v) {
    for (int q = 0; q < x.nq; q++) {
        const KLane L = klane_at(a.N, q);
        if (!L.ok) continue;
        const SoftStage s = x.st[L.k];
        if (L.c < s.nb) {
            const int lo = s.oC + L.c, up = lo + s.pnb;
            const double ltl = v.lamt[lo], ltu = v.lamt[up];
            const double lal = ltl * (1.0 / v.tinv[lo]), lau = ltu * (1.0 / v.tinv[up]);
            v.qx[L.k * V16 + L.c] = lau - ltu * v.d[s.oD + s.pnb + L.c] - lal - ltl * v.d[s.oD + L.c];
        } else if (L.c < s.nb + s.ns) {
            const SoftBox B = soft_box(v, s, L.c - s.nb);
            const double rqx0 = B.rqx0 - B.lt[0] * B.zl0 * B.Zl0;
            const double rqx1 = B.rqx1 - B.lt[1] * B.zl1 * B.Zl1;
            v.qx[L.k * V16 + L.c] = rqx1 - rqx0;
        }
    }
}

// The element-wise pass of soft_alpha at step 1: t' from ux', the slacks from (zl -+ Lam ux') Zl, lam' = Lam (tau - t').
// No step length, no positivity
__device__ inline void kkt_point(const KArgs& a, const SoftKktArgs& x, const SetView& v) {
    for (int q = 0; q < x.nq; q++) {
        const KLane L = klane_at(a.N, q);
        if (!L.ok) continue;
        const SoftStage s = x.st[L.k];
        if (L.c < s.nb) {
            const int lo = s.oC + L.c, up = lo + s.pnb;
            const double w = v.ux[L.k * V16 + x.idxb[L.k * 16 + L.c]];
            const double tl = w - v.d[s.oD + L.c], tu = v.d[s.oD + s.pnb + L.c] - w;
            v.t[lo] = tl;
            v.t[up] = tu;
            v.lam[lo] = v.lamt[lo] * (1.0 / v.tinv[lo] - tl);
            v.lam[up] = v.lamt[up] * (1.0 / v.tinv[up] - tu);
        } else if (L.c < s.nb + s.ns) {
            const int i = L.c - s.nb, pns = s.pns, b0 = s.oC + 2 * s.pnb + i;
            const SoftBox B = soft_box(v, s, i);
            const double w = v.ux[L.k * V16 + x.idxb[L.k * 16 + L.c]];
            double tn[4];
            tn[2] = (B.zl0 - B.lt[0] * w) * B.Zl0;
            tn[3] = (B.zl1 + B.lt[1] * w) * B.Zl1;
            tn[0] = tn[2] + w - v.d[s.oD + 2 * s.pnb + i];
            tn[1] = tn[3] - w + v.d[s.oD + 2 * s.pnb + pns + i];
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int e = b0 + j * pns;
                v.t[e] = tn[j];
                v.lam[e] = B.lt[j] * (B.tau[j] - tn[j]);
            }
        }
    }
}

}  // namespace

template <class FX>
__global__ __launch_bounds__(64) void hk_soft_kkt_factor(KArgs a, SoftKktArgs x) {
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int p = blockIdx.x + a.p0;
    if (p >= a.nprob) return;
    kkt_lin(a, x, opaque_prob(p));
    wsync();
    {
        const int q = opaque_prob(p);
        double* W = a.ws + (long)q * a.sW;
        RicIO io = make_io(a, T, q, W);
        BoxCtx bc{};
        bc.Qx = W + x.oVQx;
        ric_backward<false, BX_GIVEN, FX, CERT_LOAD>(io, &sm, 0, nullptr, 0, nullptr, bc, 0, nullptr);
    }
}

template <class FX>
__global__ __launch_bounds__(64) void hk_soft_kkt_rhs(KArgs a, SoftKktArgs x) {
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int j = blockIdx.x;
    const int p = a.p0 + j / x.nrhs;
    if (p >= a.nprob) return;
    const int r = j % x.nrhs;
    {
        const SetView v = set_view(a, x, opaque_prob(p), opaque_prob(r));
        kkt_gradient(a, x, v);
    }
    wsync();
    {
        const int q = opaque_prob(p);
        const long s = (long)q * x.nrhs + opaque_prob(r);
        RicIO io = make_io(a, T, q, a.ws + (long)q * a.sW);  // the factor: read only
        const long o16 = s * a.sV16;
        double* S = x.scratch + s * x.sS;
        BoxCtx bc{};
        bc.qx = S;
        double al = 1.0;
        ric_trs<BX_GIVEN, BX_NONE, FX>(io, &sm, a.vb + o16, a.vq + o16, bc, a.ux + o16, a.compute_mult, a.pi + o16, 1,
                                       S + (long)(a.N + 1) * V16, al);
    }
    wsync();
    {
        const SetView v = set_view(a, x, opaque_prob(p), opaque_prob(r));
        kkt_point(a, x, v);
    }
}

__global__ __launch_bounds__(256) void hk_ocp_soft_kkt_pack(OcpSoftKktPackArgs a) {
    const unsigned groups = (a.N + 4) / 4;
    const unsigned si = blockIdx.x / groups;
    // the wavefront's stage, as a scalar: the masked loads take wave-uniform bases
    const int k = (blockIdx.x % groups) * 4 + __builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    if (si >= (unsigned)a.count * (unsigned)a.nrhs || k > a.N) return;
    const long s = (long)a.p0 * a.nrhs + si;
    if (s >= (long)a.nprob * a.nrhs) return;
    const OcpSoftStage st = a.st[k];
    const OcpStage& o = st.o;
    const int l = threadIdx.x & 63;
    const auto at = [&](const double* p, long long n) { return p ? p + s * n : nullptr; };
    const OcpVecs vec{at(a.b, a.nb_), at(a.q, a.nq_), at(a.r, a.nr_), nullptr, nullptr, nullptr, nullptr};
    const double *lb = at(a.lb, a.nl_), *ub = at(a.ub, a.nl_), *zi = at(a.z, a.nz_);
    const int nb = o.nb, pnb = o.pnb, ns = st.ns, pns = st.pns;
    const int nd = 2 * pnb + 2 * pns, nz = zi ? 2 * pns : 0;
    double* W = a.work + s * a.sWk;
    const long n16 = (long)(a.N + 1) * V16;
    for (int e = l; e < 2 * V16 + nd + nz; e += 64) {
        if (e < 2 * V16) {  // b_k (state order), then [r_k | q_k] (variable order), padding as zeros
            const double v = __longlong_as_double(ocp_seed_bits(o, vec, e));
            W[(e < V16 ? 0 : n16) + k * V16 + (e & 15)] = v;
            continue;
        }
        // d_k = [lb pnb | ub pnb | ls pns | us pns], the soft bounds at lb / ub [nb + i]; z_k = [lower pns | upper pns]
        const int c = e - 2 * V16, c1 = c - pnb, c2 = c - 2 * pnb, c3 = c2 - pns, cz = c - nd;
        const int hz = cz >= pns ? 1 : 0, iz = cz - hz * pns;
        const double w[5] = {hk::gld(lb, o.dn[OCP_lb] + c, lb && c < nb),
                             hk::gld(ub, o.dn[OCP_ub] + c1, ub && c1 >= 0 && c1 < nb),
                             hk::gld(lb, o.dn[OCP_lb] + nb + c2, lb && c2 >= 0 && c2 < ns),
                             hk::gld(ub, o.dn[OCP_ub] + nb + c3, ub && c3 >= 0 && c3 < ns),
                             hk::gld(zi, st.dnZ + hz * ns + iz, zi && cz >= 0 && iz < ns)};
        long long bits = 0;
#pragma unroll
        for (int i = 0; i < 5; i++) bits |= __double_as_longlong(w[i]);
        const double v = __longlong_as_double(bits);
        if (c < nd)
            W[a.oD + st.oD + c] = v;
        else
            W[a.oZ + st.oZ + cz] = v;
    }
}

// Both launches of a call pass the launch guard (hk_launch_guard.h: LDS tables, private segment against the stack
// limit, launch bound) before the first is issued, so a refused call writes nothing.  The compiled inner-stage class is
// the tile plan's (KArgs.fixcls), as in hk_launch.
extern "C" int hk_soft_kkt_launch(const KArgs* a, const SoftKktArgs* x, int count, int refactor, hipStream_t stream) {
    if (count <= 0 || x->nrhs <= 0) return 0;
    return with_fixcls(a->fixcls, [&](auto fx) {
        using FX = typename decltype(fx)::type;
        static const HkKernelLimits lim_f(reinterpret_cast<const void*>(&hk_soft_kkt_factor<FX>));
        static const HkKernelLimits lim_r(reinterpret_cast<const void*>(&hk_soft_kkt_rhs<FX>));
        const size_t lds = lds_table_bytes(a->N);
        if (refactor)
            if (const int e = lim_f.check(lds, 64)) return e;
        if (const int e = lim_r.check(lds, 64)) return e;
        if (refactor) {
            hipLaunchKernelGGL(hk_soft_kkt_factor<FX>, dim3((unsigned)count), dim3(64), lds, stream, *a, *x);
            if (const int e = (int)hipGetLastError()) return e;
        }
        hipLaunchKernelGGL(hk_soft_kkt_rhs<FX>, dim3((unsigned)count * (unsigned)x->nrhs), dim3(64), lds, stream, *a,
                           *x);
        return (int)hipGetLastError();
    });
}

extern "C" int hk_ocp_soft_kkt_pack_launch(const OcpSoftKktPackArgs* a, hipStream_t stream) {
    if (a->count <= 0 || a->nrhs <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_soft_kkt_pack));
    if (const int e = lim.check(0, 256)) return e;
    const long long blocks = (long long)a->count * a->nrhs * ((a->N + 4) / 4);
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    hipLaunchKernelGGL(hk_ocp_soft_kkt_pack, dim3((unsigned)blocks), dim3(256), 0, stream, *a);
    return (int)hipGetLastError();
}

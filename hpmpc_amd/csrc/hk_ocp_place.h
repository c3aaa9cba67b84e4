// hk_ocp_place.h -- where the OCP front end's dense vectors sit in the solver's padded stage vectors, and back: one
// definition of each placement for hk_ocp_pack, hk_ocp_pack_vectors, hk_ocp_unpack (hk_ocp.hip) and the dense prologue
// and epilogue of hk_kkt_tan (hk_tan.hip), the transposes of both for those of hk_kkt_adj (hk_adj.hip), and the slots
// hk_ocp_matgrad (hk_matgrad.hip) and hk_ocp_matdir (hk_matdir.hip) read by dense index.  Device code only; lane l of a
// wavefront owns one element.
//
// In: stage k's seed row, 64 doubles -- lanes 0..15 b_k (state order), 16..31 [r_k | q_k] (variable order), 32..63 d_k =
// [lb pnb | ub pnb | lg png | ug png]; and the warm start ux_k = [u0_k | x0_k | 0 ..].
// Out: u / x from ux_k (with the equality-box fix where asked for), pi from pi_k, compact lam / t from the padded slots.
#pragma once
#include "hk_ocp_args.h"
#include "hk_prims.h"
#include "hpmpc_kargs.h"

namespace {

// The dense vector arrays of one problem or set, already offset to it (null: zeros).
struct OcpVecs {
    const double *b, *q, *r, *lb, *ub, *lg, *ug;
};

// Element c of d_k, and lane l's element of the seed row: zero for padding and for a null array.  Every source is
// loaded with its own wave-uniform base and a lane mask (a masked lane reads zero bits), and the loads are OR-ed:
// at most one is live per lane, there is no branch, and the loads of several stages overlap.
__device__ __forceinline__ long long ocp_d_bits(const OcpStage& s, const OcpVecs& v, int c) {
    const int cu = c - s.pnb, cg = c - 2 * s.pnb, ch = c - 2 * s.pnb - s.png;
    const double w[4] = {hk::gld(v.lb, s.dn[OCP_lb] + c, v.lb && c >= 0 && c < s.nb),
                         hk::gld(v.ub, s.dn[OCP_ub] + cu, v.ub && cu >= 0 && cu < s.nb),
                         hk::gld(v.lg, s.dn[OCP_lg] + cg, v.lg && cg >= 0 && cg < s.ng),
                         hk::gld(v.ug, s.dn[OCP_ug] + ch, v.ug && ch >= 0 && ch < s.ng)};
    long long bits = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) bits |= __double_as_longlong(w[i]);
    return bits;
}
__device__ __forceinline__ long long ocp_seed_bits(const OcpStage& s, const OcpVecs& v, int l) {
    const int e = l & 15;
    const bool isb = l < 16, isq = l >= 16 && l < 32;
    const double w[3] = {hk::gld(v.b, s.dn[OCP_b] + e, isb && v.b && e < s.nx1),
                         hk::gld(v.r, s.dn[OCP_r] + e, isq && v.r && e < s.nu),
                         hk::gld(v.q, s.dn[OCP_q] + (e - s.nu), isq && v.q && e >= s.nu && e < s.nu + s.nx)};
    long long bits = ocp_d_bits(s, v, l - 32);
#pragma unroll
    for (int i = 0; i < 3; i++) bits |= __double_as_longlong(w[i]);
    return bits;
}

// Element e of the warm start ux_k, from u0 / x0 shaped like r / q.
__device__ __forceinline__ double ocp_warm_elem(const OcpStage& s, const double* u0, const double* x0, int e) {
    if (e < s.nu) return u0[s.dn[OCP_r] + e];
    return e < s.nu + s.nx ? x0[s.dn[OCP_q] + (e - s.nu)] : 0.0;
}

// Slot of compact constraint element l ([lb nb | ub nb | lg ng | ug ng]) in the padded V32 stage vector.
__device__ __forceinline__ int compact_src(const OcpStage& s, int l) {
    if (l < s.nb) return l;
    if (l < 2 * s.nb) return s.pnb + (l - s.nb);
    if (l < 2 * s.nb + s.ng) return 2 * s.pnb + (l - 2 * s.nb);
    return 2 * s.pnb + s.png + (l - 2 * s.nb - s.ng);
}

// The outputs of set s.
__device__ __forceinline__ OcpOut ocp_out_at(const OcpOut& o, long s) {
    return {o.u + s * o.su, o.x + s * o.sx, o.pi + s * o.sp, o.lam + s * o.sl, o.t ? o.t + s * o.sl : nullptr,
            o.su, o.sx, o.sp, o.sl};
}

// Lane l's stores of stage k: ux -> u or x, pi, and lam / t (read from slot compact_src) -> compact element l.  With dk
// (the stage's padded d) and ik (its 16 box indices) the equality-box fix over the leading input boxes is applied:
// u[idxb[j]] = lb[j] where lb[j] == ub[j].
__device__ __forceinline__ void ocp_unpack_store(const OcpStage& s, const OcpOut& o, int l, double ux, double pi,
                                                 double lam, double t, const double* dk = nullptr,
                                                 const int* ik = nullptr) {
    if (l < s.nu) {
        if (dk)
            for (int j = 0; j < s.nbu; j++) {
                const double lo = dk[j], up = dk[s.pnb + j];
                if (ik[j] == l && lo == up) ux = lo;
            }
        o.u[s.dn[OCP_r] + l] = ux;
    } else if (l < s.nu + s.nx) {
        o.x[s.dn[OCP_q] + (l - s.nu)] = ux;
    }
    if (l < s.nx1) o.pi[s.dn[OCP_b] + l] = pi;
    if (l < 2 * s.nb + 2 * s.ng) {
        const int e = 2 * s.dn[OCP_lb] + 2 * s.dn[OCP_lg] + l;
        o.lam[e] = lam;
        if (o.t) o.t[e] = t;
    }
}

// ---- the adjoint's placements (hk_kkt_adj, hk_adj.hip): the transposes of the two above ----

// The dense cotangents of one set, already offset to it (null: zeros): u, x, pi shaped like r, q, b, lam / t compact.
struct OcpCots {
    const double *u, *x, *pi, *lam, *t;
};

// Padded slot c of a compact constraint array `a` (lam or t), the transpose of ocp_unpack_store's gather through
// compact_src: zero bits for padding, a slot out of range and a null array.
__device__ __forceinline__ long long ocp_compact_bits(const OcpStage& s, const double* a, int c) {
    const int cu = c - s.pnb, cg = c - 2 * s.pnb, ch = c - 2 * s.pnb - s.png;
    const int base = 2 * s.dn[OCP_lb] + 2 * s.dn[OCP_lg];
    const double w[4] = {hk::gld(a, base + c, a && c >= 0 && c < s.nb),
                         hk::gld(a, base + s.nb + cu, a && cu >= 0 && cu < s.nb),
                         hk::gld(a, base + 2 * s.nb + cg, a && cg >= 0 && cg < s.ng),
                         hk::gld(a, base + 2 * s.nb + s.ng + ch, a && ch >= 0 && ch < s.ng)};
    long long bits = 0;
#pragma unroll
    for (int i = 0; i < 4; i++) bits |= __double_as_longlong(w[i]);
    return bits;
}
// Lane l's element of stage k's cotangent row, the transpose of ocp_unpack_store without the equality-box fix: lanes
// 0..15 gpi_k (state order), 16..31 gux_k = [gu_k | gx_k] (variable order), 32..63 the padded glam_k.  The padded gt_k
// is ocp_compact_bits(s, g.t, l - 32).  OR-ed masked loads, as in ocp_seed_bits.
__device__ __forceinline__ long long ocp_cot_bits(const OcpStage& s, const OcpCots& g, int l) {
    const int e = l & 15;
    const bool isp = l < 16, isv = l >= 16 && l < 32;
    const double w[3] = {hk::gld(g.pi, s.dn[OCP_b] + e, isp && g.pi && e < s.nx1),
                         hk::gld(g.u, s.dn[OCP_r] + e, isv && g.u && e < s.nu),
                         hk::gld(g.x, s.dn[OCP_q] + (e - s.nu), isv && g.x && e >= s.nu && e < s.nu + s.nx)};
    long long bits = ocp_compact_bits(s, g.lam, l - 32);
#pragma unroll
    for (int i = 0; i < 3; i++) bits |= __double_as_longlong(w[i]);
    return bits;
}

// The dense gradients of one set, already offset to it (null: not wanted), shaped like the data arrays.
struct OcpGrads {
    double *b, *q, *r, *lb, *ub, *lg, *ug;
};

// Whether lane l's slot of the 64-double stage row [state order (16) | variable order (16) | d_k (32)] carries an
// element (not padding).
__device__ __forceinline__ bool ocp_row_live(const OcpStage& s, int l) {
    const int e = l & 15, c = l - 32;
    const int cu = c - s.pnb, cg = c - 2 * s.pnb, ch = c - 2 * s.pnb - s.png;
    if (l < 16) return e < s.nx1;
    if (l < 32) return e < s.nu + s.nx;
    return c < s.nb || (cu >= 0 && cu < s.nb) || (cg >= 0 && cg < s.ng) || (ch >= 0 && ch < s.ng);
}

// Lane l's store of stage k's gradient row [bbar_k (16) | qbar_k (16) | dbar_k (32)]: the exact transpose of
// ocp_seed_bits, which copies each dense element to one slot with unit weight -- so each slot goes back to that
// element, unscaled, and padding slots go nowhere.
__device__ __forceinline__ void ocp_grad_store(const OcpStage& s, const OcpGrads& o, int l, double v) {
    const int e = l & 15, c = l - 32;
    const int cu = c - s.pnb, cg = c - 2 * s.pnb, ch = c - 2 * s.pnb - s.png;
    if (l < 16) {
        if (o.b && e < s.nx1) o.b[s.dn[OCP_b] + e] = v;
    } else if (l < 32) {
        if (o.r && e < s.nu) o.r[s.dn[OCP_r] + e] = v;
        if (o.q && e >= s.nu && e < s.nu + s.nx) o.q[s.dn[OCP_q] + (e - s.nu)] = v;
    } else {
        if (o.lb && c < s.nb) o.lb[s.dn[OCP_lb] + c] = v;
        if (o.ub && cu >= 0 && cu < s.nb) o.ub[s.dn[OCP_ub] + cu] = v;
        if (o.lg && cg >= 0 && cg < s.ng) o.lg[s.dn[OCP_lg] + cg] = v;
        if (o.ug && ch >= 0 && ch < s.ng) o.ug[s.dn[OCP_ug] + ch] = v;
    }
}

// ---- by dense index (hk_ocp_matgrad, hk_matgrad.hip; hk_ocp_matdir, hk_matdir.hip): the slot of input j / state j in the V16 stage vector in
// variable order [u | x], and of general constraint l's lower / upper side in the V32 stage vector ----
__device__ __forceinline__ int ocp_slot_u(const OcpStage&, int j) { return j; }
__device__ __forceinline__ int ocp_slot_x(const OcpStage& s, int j) { return s.nu + j; }
__device__ __forceinline__ int ocp_slot_lg(const OcpStage& s, int l) { return 2 * s.pnb + l; }
__device__ __forceinline__ int ocp_slot_ug(const OcpStage& s, int l) { return 2 * s.pnb + s.png + l; }
// and back (hk_ocp_matdir, hk_matdir.hip, whose lane l owns slot l of the seed row): the input / state of slot v of the
// V16 vector in variable order, the general constraint of slot c of the V32 vector's lower / upper side; -1: none
__device__ __forceinline__ int ocp_u_of_slot(const OcpStage& s, int v) { return v >= 0 && v < s.nu ? v : -1; }
__device__ __forceinline__ int ocp_x_of_slot(const OcpStage& s, int v) {
    return v >= s.nu && v < s.nu + s.nx ? v - s.nu : -1;
}
__device__ __forceinline__ int ocp_lg_of_slot(const OcpStage& s, int c) {
    const int g = c - 2 * s.pnb;
    return g >= 0 && g < s.ng ? g : -1;
}
__device__ __forceinline__ int ocp_ug_of_slot(const OcpStage& s, int c) {
    const int g = c - 2 * s.pnb - s.png;
    return g >= 0 && g < s.ng ? g : -1;
}

}  // namespace

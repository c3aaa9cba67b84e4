// hk_adj.hip -- MI355X (gfx950): the batched KKT adjoint solve (hpmpc_mi355x_kkt_adjoint_batch,
// hpmpc_mi355x_ocp_adjoint_batch).
//
// hk_kkt_adj: one wavefront per (problem, cotangent set), grid = count * nadj, set index s = p * nadj + r exactly as in
// hk_kkt_tan (hk_tan.hip).  It applies the transpose of the tangent map (hk_adj_body.h): reverse-mode sensitivities of
// the re-solved iterate, the gradient of one scalar loss with respect to every element of (b, q, d) per set.  The sets
// of a problem share its stage data and the workspace an IPM left (F, t_inv, lam_bkp: read only, never stored to).
// The work vectors live in the set's block of the caller's scratch, in the carve of hk_kkt_rhs; every element read
// there is written first.
//
// Two front ends, one kernel.  Padded: the cotangents are the caller's V16 / V32 arrays, read in place (a null V16 one
// is replaced by a zero vector in the scratch, a null V32 one is read as zero), and the gradients go straight to the
// caller's padded arrays.  Dense (AdjArgs.ost, the OCP call): the prologue scatters the dense cotangents u, x, pi and
// the compact lam, t into the scratch's padded vectors -- the transpose of hk_ocp_unpack's placement, without the
// equality-box fix -- the body leaves bbar / qbar / dbar in the scratch, and the epilogue gathers them into the dense
// shapes of b, q, r, lb, ub, lg, ug: the transpose of hk_ocp_pack_vectors' placement (hk_ocp_place.h).
#include "hk_adj_args.h"
#include "hk_adj_body.h"
#include "hk_kkt_launch.h"
#include "hk_launch.h"
#include "hk_ocp_place.h"

namespace {

// Stages per batch of the dense prologue and epilogue, as in hk_kkt_tan: the loads of ADJ_CH stages are issued
// before any is stored.
constexpr int ADJ_CH = 4;

}  // namespace

template <class FX>
__global__ __launch_bounds__(64) void hk_kkt_adj(KArgs a, AdjArgs x) {
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int j = blockIdx.x;
    const int p = a.p0 + j / x.k.nrhs;
    if (p >= a.nprob) return;
    const long s = (long)p * x.k.nrhs + j % x.k.nrhs;
    const int N = a.N;
    const int l = lane_id();
    const Ws w = carve(a.ws + (long)p * a.sW, N);  // read only: F, t_inv and lam_bkp
    const long n16 = (long)(N + 1) * V16;
    const KktSet c = carve_set(x.k.scratch + s * x.k.sS, N);  // this set's scratch block, as in hk_kkt_rhs
    AdjIO v;
    v.qx = c.qx;
    v.Pb = c.Pb;
    v.zero = c.res_m;
    v.z = c.dt;
    v.zl = c.dlam;
    v.t_inv = w.t_inv;
    v.lam_bkp = w.lam_bkp;
    const bool dense = x.ost != nullptr;
    const long o16 = s * a.sV16, o32 = s * a.sV32;
    if (dense) {
        // prologue.  Lanes 0..15 gpi_k -> res_b, 16..31 [gu_k | gx_k] -> res_q, 32..63 glam_k -> dt and gt_k -> dlam (both
        // are consumed by the body's first pass, before the solve's general half overwrites them); every element of
        // the four vectors is written, zero where the cotangent is null or the slot is padding
        const auto in = [&](int i) -> const double* { return x.cot[i].p ? x.cot[i].p + s * x.cot[i].s : nullptr; };
        const OcpCots g{in(0), in(1), in(2), in(3), in(4)};
        for (int k0 = 0; k0 <= N; k0 += ADJ_CH) {
            long long row[ADJ_CH], tb[ADJ_CH];
#pragma unroll
            for (int j = 0; j < ADJ_CH; j++) {
                const int k = k0 + j <= N ? k0 + j : N;  // clamped: the stores below are masked
                row[j] = ocp_cot_bits(x.ost[k], g, l);
                tb[j] = ocp_compact_bits(x.ost[k], g.t, l - 32);
            }
#pragma unroll
            for (int j = 0; j < ADJ_CH; j++) {
                const int k = k0 + j;
                double* dst = l < 16 ? c.res_b + k * V16 + l : l < 32 ? c.res_q + k * V16 + (l - 16) : c.dt + k * V32 + (l - 32);
                if (k <= N) {
                    *dst = __longlong_as_double(row[j]);
                    if (l >= 32) c.dlam[k * V32 + (l - 32)] = __longlong_as_double(tb[j]);
                }
            }
        }
        v.gpi = c.res_b;
        v.gux = c.res_q;
        v.glam = c.dt;
        v.gt = c.dlam;
        v.qbar = c.dux;
        v.bbar = c.dpi;
        v.dbar = c.res_d;
    } else {
        // a null V16 cotangent is a zero vector of the scratch; a given one is read in place
        if (!a.vb)
            for (int i = l; i < n16; i += 64) c.res_b[i] = 0.0;
        if (!a.vq)
            for (int i = l; i < n16; i += 64) c.res_q[i] = 0.0;
        v.gpi = a.vb ? a.vb + o16 : c.res_b;
        v.gux = a.vq ? a.vq + o16 : c.res_q;
        v.glam = x.glam ? x.glam + o32 : nullptr;
        v.gt = x.gt ? x.gt + o32 : nullptr;
        v.qbar = a.ux + o16;
        v.bbar = a.pi ? a.pi + o16 : c.dpi;  // not stored to without compute_mult
        v.dbar = a.lam + o32;
    }
    wsync();
    RicIO io = make_io(a, T, p, w.F);
    BoxTab bt{T.tileslot, T.slotvar};
    adj_body<FX>(a, io, &sm, bt, v, !dense);  // dense: the epilogue reads only elements the body defines
    if (!dense) return;
    wsync();
    // epilogue: the transpose of hk_ocp_pack_vectors' placement
    OcpGrads o;
    {
        const auto out = [&](int i) -> double* { return x.grad.p[i] ? x.grad.p[i] + s * x.grad.s[i] : nullptr; };
        o = OcpGrads{out(OCP_b), out(OCP_q), out(OCP_r), out(OCP_lb), out(OCP_ub), out(OCP_lg), out(OCP_ug)};
    }
    for (int k0 = 0; k0 <= N; k0 += ADJ_CH) {
        double g[ADJ_CH];
#pragma unroll
        for (int j = 0; j < ADJ_CH; j++) {
            const int k = k0 + j <= N ? k0 + j : N;  // clamped: the stores below are masked
            const bool live = ocp_row_live(x.ost[k], l) && (l >= 16 || a.compute_mult);
            const double* src = l < 16 ? v.bbar : l < 32 ? v.qbar : v.dbar;
            const int e = l < 16 ? k * V16 + l : l < 32 ? k * V16 + (l - 16) : k * V32 + (l - 32);
            g[j] = live ? src[e] : 0.0;
        }
#pragma unroll
        for (int j = 0; j < ADJ_CH; j++) {
            if (k0 + j <= N) ocp_grad_store(x.ost[k0 + j], o, l, g[j]);
        }
    }
}

extern "C" int hk_kkt_adj_launch(const KArgs* a, const AdjArgs* x, int count, hipStream_t stream) {
    return kkt_sets_launch(a, x, count, x->k.nrhs, stream,
                           [](auto fx) { return &hk_kkt_adj<typename decltype(fx)::type>; });
}

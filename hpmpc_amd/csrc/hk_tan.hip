// hk_tan.hip -- MI355X (gfx950): the batched KKT tangent solve (hpmpc_mi355x_kkt_tangent_batch,
// hpmpc_mi355x_ocp_tangent_batch).
//
// hk_kkt_tan: one wavefront per (problem, direction), grid = count * ndir, set index s = p * ndir + r exactly as in
// hk_kkt_rhs (hk_kkt.hip).  It computes the linear part of the re-solve map in (b, q, d) directly (hk_tan_body.h):
// forward sensitivities of the re-solved iterate, one set per parameter direction.  The sets of a problem share its
// stage data and the workspace an IPM left (F, t_inv, lam_bkp: read only, never stored to).  The work vectors live in
// the set's block of the caller's scratch, in the carve of hk_kkt_rhs; every element read there is written first.
//
// Two front ends, one kernel.  Padded: the directions are the caller's V16 / V32 arrays, read in place (a null one
// is replaced by a zero vector in the scratch), and the results go straight to the caller's padded arrays.  Dense
// (TanArgs.ost, the OCP call): the prologue seeds res_b / res_q / res_d of the scratch from the dense directions, the
// body leaves its results in the scratch's dux / dpi / dlam / dt, and the epilogue writes them out in the dense OCP
// shapes -- hk_ocp_pack_vectors' and hk_ocp_unpack's placements (hk_ocp_place.h) without a launch or a padded array
// of their own.  The equality-box fix of hk_ocp_unpack is NOT applied: the tangent of a variable pinned by lb == ub is
// whatever the Newton system gives (zero up to the rounding of 1 / t), not a copy of the bound's direction.
#include "hk_kkt_launch.h"
#include "hk_launch.h"
#include "hk_ocp_place.h"
#include "hk_tan_args.h"
#include "hk_tan_body.h"

namespace {

// Stages per batch of the dense prologue and epilogue: the loads of TAN_CH stages are issued before any is stored,
// so a set pays a memory round trip per batch and not per stage.
constexpr int TAN_CH = 4;

}  // namespace

// SEEDED (dense mode only; hpmpc_mi355x_ocp_tangent_data_batch): res_b / res_q / res_d of the scratch already hold the
// seed rows -- hk_ocp_matdir (hk_matdir.hip) wrote them earlier on the stream -- and the prologue is skipped.
template <class FX, bool SEEDED = false>
__global__ __launch_bounds__(64) void hk_kkt_tan(KArgs a, TanArgs x) {
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int j = blockIdx.x;
    const int p = a.p0 + j / x.k.nrhs;
    if (p >= a.nprob) return;
    const long s = (long)p * x.k.nrhs + j % x.k.nrhs;
    const int N = a.N;
    const int l = lane_id();
    const Ws w = carve(a.ws + (long)p * a.sW, N);  // read only: F, t_inv and lam_bkp
    const long n16 = (long)(N + 1) * V16, n32 = (long)(N + 1) * V32;
    const KktSet c = carve_set(x.k.scratch + s * x.k.sS, N);  // this set's scratch block, as in hk_kkt_rhs
    double *res_q = c.res_q, *res_b = c.res_b, *res_d = c.res_d;
    TanIO v;
    v.qx = c.qx;
    v.Pb = c.Pb;
    v.res_m = c.res_m;
    v.t_inv = w.t_inv;
    v.lam_bkp = w.lam_bkp;
    const bool dense = x.ost != nullptr;
    const long o16 = s * a.sV16, o32 = s * a.sV32;
    if (dense) {
        // prologue: hk_ocp_pack_vectors' placement.  Lanes 0..15 db_k (state order), 16..31 [dr_k | dq_k], 32..63 dd_k;
        // every element of the three vectors is written, zero where the direction is null or the slot is padding
        const auto in = [&](int i) -> const double* { return x.in[i].p ? x.in[i].p + s * x.in[i].s : nullptr; };
        const OcpVecs dir{in(OCP_b), in(OCP_q), in(OCP_r), in(OCP_lb), in(OCP_ub), in(OCP_lg), in(OCP_ug)};
        for (int k0 = 0; !SEEDED && k0 <= N; k0 += TAN_CH) {
            long long bits[TAN_CH];
#pragma unroll
            for (int j = 0; j < TAN_CH; j++) {
                const int k = k0 + j <= N ? k0 + j : N;  // clamped: the store below is masked
                bits[j] = ocp_seed_bits(x.ost[k], dir, l);
            }
#pragma unroll
            for (int j = 0; j < TAN_CH; j++) {
                const int k = k0 + j;
                double* dst = l < 16 ? res_b + k * V16 + l : l < 32 ? res_q + k * V16 + (l - 16) : res_d + k * V32 + (l - 32);
                if (k <= N) *dst = __longlong_as_double(bits[j]);
            }
        }
        v.hb = res_b;
        v.hq = res_q;
        v.rd = res_d;
        v.dux = c.dux;
        v.dpi = c.dpi;
        v.dt = c.dt;
        v.dlam = c.dlam;
    } else {
        // a null direction is a zero vector of the scratch; a given one is read in place
        if (!a.vb)
            for (int i = l; i < n16; i += 64) res_b[i] = 0.0;
        if (!a.vq)
            for (int i = l; i < n16; i += 64) res_q[i] = 0.0;
        if (!a.d)
            for (int i = l; i < n32; i += 64) res_d[i] = 0.0;
        v.hb = a.vb ? a.vb + o16 : res_b;
        v.hq = a.vq ? a.vq + o16 : res_q;
        v.rd = a.d ? a.d + o32 : res_d;
        v.dux = a.ux + o16;
        v.dpi = a.pi + o16;
        v.dlam = a.lam + o32;
        v.dt = a.t + o32;
    }
    wsync();
    RicIO io = make_io(a, T, p, w.F);
    BoxTab bt{T.tileslot, T.slotvar};
    tan_body<FX>(a, io, &sm, bt, v, !dense);  // dense: the epilogue reads only elements the solve defines
    if (!dense) return;
    wsync();
    // epilogue: hk_ocp_unpack's placement, without the equality-box fix and without residuals
    const OcpOut o = ocp_out_at(x.out, s);
    for (int k0 = 0; k0 <= N; k0 += TAN_CH) {
        double ux[TAN_CH], pv[TAN_CH], lm[TAN_CH], tv[TAN_CH];
#pragma unroll
        for (int j = 0; j < TAN_CH; j++) {
            const int k = k0 + j <= N ? k0 + j : N;  // clamped: the stores below are masked
            const OcpStage& os = x.ost[k];
            const bool cv = l < 2 * os.nb + 2 * os.ng;
            const int src = k * V32 + compact_src(os, cv ? l : 0);
            ux[j] = gld(v.dux, k * V16 + l, l < os.nu + os.nx);
            pv[j] = gld(v.dpi, k * V16 + l, k < N && l < os.nx1);
            lm[j] = gld(v.dlam, src, cv);
            tv[j] = gld(v.dt, src, cv);
        }
#pragma unroll
        for (int j = 0; j < TAN_CH; j++) {
            if (k0 + j <= N) ocp_unpack_store(x.ost[k0 + j], o, l, ux[j], pv[j], lm[j], tv[j]);
        }
    }
}

extern "C" int hk_kkt_tan_launch(const KArgs* a, const TanArgs* x, int count, hipStream_t stream) {
    return kkt_sets_launch(a, x, count, x->k.nrhs, stream,
                           [](auto fx) { return &hk_kkt_tan<typename decltype(fx)::type>; });
}

extern "C" int hk_kkt_tan_seeded_launch(const KArgs* a, const TanArgs* x, int count, hipStream_t stream) {
    if (!x->ost) return -1;  // the padded front end reads its directions in place: nothing to seed
    return kkt_sets_launch(a, x, count, x->k.nrhs, stream,
                           [](auto fx) { return &hk_kkt_tan<typename decltype(fx)::type, true>; });
}

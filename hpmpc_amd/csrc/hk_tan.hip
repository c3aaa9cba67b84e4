// hk_tan.hip -- MI355X (gfx950): the batched KKT tangent solve (hpmpc_mi355x_kkt_tangent_batch,
// hpmpc_mi355x_ocp_tangent_batch) and the multi-set OCP finish (hpmpc_mi355x_ocp_unpack_sets).
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
// shapes -- hk_ocp_pack_vectors' and hk_ocp_finish's placements without a launch or a padded array of their own.
// The equality-box fix of hk_ocp_finish is NOT applied: the tangent of a variable pinned by lb == ub is whatever
// the Newton system gives (zero up to the rounding of 1 / t), not a copy of the bound's direction.
//
// hk_ocp_unpack_sets: hk_ocp_finish's data movement for nprob * nrhs re-solved sets (one wavefront per set): dense u,
// x, pi, compact lam / t, with the equality-box fix from the set's own d.  No residuals.
#include "hk_launch.h"
#include "hk_tan_args.h"
#include "hk_tan_body.h"

namespace {

// Stages per batch of the dense prologue and epilogue: the loads of TAN_CH stages are issued before any is stored,
// so a set pays a memory round trip per batch and not per stage.
constexpr int TAN_CH = 4;

// The dense directions of one set (null: a zero direction), already offset to the set.
struct TanDirs {
    const double *b, *q, *r, *lb, *ub, *lg, *ug;
};

// Lane l's element of stage k's seed row [db_k (16, state order) | dr_k, dq_k (16, variable order) | dd_k (32, as
// lb pnb | ub pnb | lg png | ug png)]: hk_ocp_pack_vectors' placement, zero for padding and for a null direction.
// Every source is loaded with its own wave-uniform base and a lane mask (a masked lane reads zero bits), and the
// loads are OR-ed: exactly one is live per lane, there is no branch, and the loads of several stages overlap.
__device__ __forceinline__ long long tan_seed_bits(const OcpStage& s, const TanDirs& d, int l) {
    const int e = l & 15, c = l - 32;
    const bool isb = l < 16, isq = l >= 16 && l < 32;
    const int cu = c - s.pnb, cg = c - 2 * s.pnb, ch = c - 2 * s.pnb - s.png;
    const double v[7] = {
        gld(d.b, s.dn[OCP_b] + e, isb && d.b && e < s.nx1),
        gld(d.r, s.dn[OCP_r] + e, isq && d.r && e < s.nu),
        gld(d.q, s.dn[OCP_q] + (e - s.nu), isq && d.q && e >= s.nu && e < s.nu + s.nx),
        gld(d.lb, s.dn[OCP_lb] + c, d.lb && c >= 0 && c < s.nb),
        gld(d.ub, s.dn[OCP_ub] + cu, d.ub && cu >= 0 && cu < s.nb),
        gld(d.lg, s.dn[OCP_lg] + cg, d.lg && cg >= 0 && cg < s.ng),
        gld(d.ug, s.dn[OCP_ug] + ch, d.ug && ch >= 0 && ch < s.ng)};
    long long bits = 0;
#pragma unroll
    for (int i = 0; i < 7; i++) bits |= __double_as_longlong(v[i]);
    return bits;
}

// slot of compact constraint element l ([lb nb | ub nb | lg ng | ug ng]) in the padded V32 stage vector
__device__ __forceinline__ int compact_src(const OcpStage& s, int l) {
    if (l < s.nb) return l;
    if (l < 2 * s.nb) return s.pnb + (l - s.nb);
    if (l < 2 * s.nb + s.ng) return 2 * s.pnb + (l - 2 * s.nb);
    return 2 * s.pnb + s.png + (l - 2 * s.nb - s.ng);
}

}  // namespace

template <class FX>
__global__ __launch_bounds__(64) void hk_kkt_tan(KArgs a, TanArgs x) {
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int j = blockIdx.x;
    const int p = a.p0 + j / x.ndir;
    if (p >= a.nprob) return;
    const long s = (long)p * x.ndir + j % x.ndir;
    const int N = a.N;
    const int l = lane_id();
    const Ws w = carve(a.ws + (long)p * a.sW, N);  // read only: F, t_inv and lam_bkp
    const long n16 = (long)(N + 1) * V16, n32 = (long)(N + 1) * V32;
    // this set's scratch block in the carve of hk_kkt_rhs: res_q, res_b, qx, dux, dpi, Pb | res_d, res_m, dt, dlam
    double* S = x.scratch + s * x.sS;
    double* res_q = S;
    double* res_b = S + n16;
    double* S32 = S + KKT_SCRATCH_V16 * n16;
    double* res_d = S32;
    TanIO v;
    v.qx = S + 2 * n16;
    v.Pb = S + 5 * n16;
    v.res_m = S32 + n32;
    v.t_inv = w.t_inv;
    v.lam_bkp = w.lam_bkp;
    const bool dense = x.ost != nullptr;
    const long o16 = s * a.sV16, o32 = s * a.sV32;
    if (dense) {
        // prologue: hk_ocp_pack_vectors' placement.  Lanes 0..15 db_k (state order), 16..31 [dr_k | dq_k], 32..63 dd_k;
        // every element of the three vectors is written, zero where the direction is null or the slot is padding
        const auto in = [&](int i) -> const double* { return x.in[i].p ? x.in[i].p + s * x.in[i].s : nullptr; };
        const TanDirs dir{in(OCP_b), in(OCP_q), in(OCP_r), in(OCP_lb), in(OCP_ub), in(OCP_lg), in(OCP_ug)};
        for (int k0 = 0; k0 <= N; k0 += TAN_CH) {
            long long bits[TAN_CH];
#pragma unroll
            for (int j = 0; j < TAN_CH; j++) {
                const int k = k0 + j <= N ? k0 + j : N;  // clamped: the store below is masked
                bits[j] = tan_seed_bits(x.ost[k], dir, l);
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
        v.dux = S + 3 * n16;
        v.dpi = S + 4 * n16;
        v.dt = S32 + 2 * n32;
        v.dlam = S32 + 3 * n32;
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
    // epilogue: hk_ocp_finish's placement, without the equality-box fix and without residuals
    double* du = x.du + s * x.su;
    double* dx = x.dx + s * x.sx;
    double* dpo = x.dpo + s * x.sp;
    double* dlo = x.dlo + s * x.sl;
    double* dto = x.dto + s * x.sl;
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
            const int k = k0 + j;
            if (k > N) continue;
            const OcpStage& os = x.ost[k];
            if (l < os.nu)
                du[os.dn[OCP_r] + l] = ux[j];
            else if (l < os.nu + os.nx)
                dx[os.dn[OCP_q] + (l - os.nu)] = ux[j];
            if (k < N && l < os.nx1) dpo[os.dn[OCP_b] + l] = pv[j];
            if (l < 2 * os.nb + 2 * os.ng) {
                const int o = 2 * os.dn[OCP_lb] + 2 * os.dn[OCP_lg] + l;
                dlo[o] = lm[j];
                dto[o] = tv[j];
            }
        }
    }
}

__global__ __launch_bounds__(64) void hk_ocp_unpack_sets(OcpSetsArgs a) {
    const unsigned j = blockIdx.x;
    const long p = (long)a.p0 + j / (unsigned)a.nrhs;
    if (j / (unsigned)a.nrhs >= (unsigned)a.count || p >= a.nprob) return;
    const long s = p * a.nrhs + j % (unsigned)a.nrhs;
    const int l = threadIdx.x;
    const double* d = a.d + s * a.sV32;
    const double* ux = a.ux + s * a.sV16;
    const double* pi = a.pi + s * a.sV16;
    const double* lam = a.lam + s * a.sV32;
    const double* t = a.t + s * a.sV32;
    double* u = a.u + s * a.su;
    double* xo = a.x + s * a.sx;
    double* po = a.po + s * a.sp;
    double* lamo = a.lamo + s * a.sl;
    double* to = a.to ? a.to + s * a.sl : nullptr;
    for (int k = 0; k <= a.N; k++) {
        const OcpStage os = a.st[k];
        if (l < os.nu + os.nx) {
            double val = ux[k * V16 + l];
            if (l < os.nu) {
                // hk_ocp_finish's equality-box fix over the leading input boxes, from the set's own d
                for (int i = 0; i < os.nbu; i++) {
                    const double lo = d[k * V32 + i], up = d[k * V32 + os.pnb + i];
                    if (a.idxb[k * 16 + i] == l && lo == up) val = lo;
                }
                u[os.dn[OCP_r] + l] = val;
            } else {
                xo[os.dn[OCP_q] + (l - os.nu)] = val;
            }
        }
        if (l < os.nx1) po[os.dn[OCP_b] + l] = pi[k * V16 + l];
        if (l < 2 * os.nb + 2 * os.ng) {
            const int src = compact_src(os, l);
            const int o = 2 * os.dn[OCP_lb] + 2 * os.dn[OCP_lg] + l;
            lamo[o] = lam[k * V32 + src];
            if (to) to[o] = t[k * V32 + src];
        }
    }
}

template <class FX>
static int kkt_tan_launch_t(const KArgs* a, const TanArgs* x, int count, hipStream_t stream) {
    // the launch guard (hk_launch_guard.h): LDS tables, private segment against the stack limit, launch bound
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_kkt_tan<FX>));
    const size_t lds = lds_table_bytes(a->N);
    if (const int e = lim.check(lds, 64)) return e;
    hipLaunchKernelGGL(hk_kkt_tan<FX>, dim3((unsigned)count * (unsigned)x->ndir), dim3(64), lds, stream, *a, *x);
    return (int)hipGetLastError();
}

// The compiled inner-stage class is the tile plan's (KArgs.fixcls), as in hk_launch.
extern "C" int hk_kkt_tan_launch(const KArgs* a, const TanArgs* x, int count, hipStream_t stream) {
    if (count <= 0 || x->ndir <= 0) return 0;
    return with_fixcls(a->fixcls, [&](auto fx) {
        return kkt_tan_launch_t<typename decltype(fx)::type>(a, x, count, stream);
    });
}

extern "C" int hk_ocp_unpack_sets_launch(const OcpSetsArgs* a, hipStream_t stream) {
    if (a->count <= 0 || a->nrhs <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_unpack_sets));
    if (const int e = lim.check(0, 64)) return e;
    const long long blocks = (long long)a->count * a->nrhs;
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    hipLaunchKernelGGL(hk_ocp_unpack_sets, dim3((unsigned)blocks), dim3(64), 0, stream, *a);
    return (int)hipGetLastError();
}

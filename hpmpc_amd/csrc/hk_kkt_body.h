// hk_kkt_body.h -- d_kkt_solve_new_rhs_res_mpc_hard_tv (mpc_solvers/d_ip2_res_hard.c:1922-2299) as a device function,
// one wavefront per call: the re-solve of an IPM's last Newton system for new b, q and bounds, on the factor, t^-1
// and the iterate backups that IPM left in its workspace.  Run by hk_kkt_new_rhs (hpmpc_kernels.hip: one problem per
// workgroup, everything in the problem's workspace) and by hk_kkt_rhs (hk_kkt.hip: many right-hand-side sets per
// problem, the workspace read only and the work vectors in a scratch of the set's own).
//
// Of the workspace carve `w` the body only READS F (through io.F), t_inv, ux_bkp, pi_bkp, lam_bkp and t_bkp, and it
// reads and writes res_q, res_b, res_d, res_m, qx, dux, dpi, Pb, dt and dlam: the caller may point these ten anywhere.
#pragma once
#include "hk_ipm_body.h"

namespace {

struct KktIO {
    const double *vb, *vq;      // the batch's b (state order) / q (variable order) arrays, V16 per stage, and where
    long o16;                   // this call's vectors start in them (doubles); NULLABLE: null = the augmented rows
    const double* d;            // bounds, V32 per stage
    double *ux, *pi, *lam, *t;  // the re-solved iterate (V16 / V16 / V32 / V32)
};

// `a`: N, ngt and compute_mult.  With compute_mult = 0 the solve leaves w.dpi as it was and pi = pi_bkp + dpi: a
// caller with a fresh dpi clears it.  NULLABLE = false is hk_kkt_new_rhs, whose b and q are always given: the body
// then compiles to that kernel's code before it was shared (the same instructions but for a few commuted operands).
template <class FX, bool NULLABLE>
__device__ __forceinline__ void kkt_body(const KArgs& a, const RicIO& io, Scratch* sm, const BoxTab& bt, const Ws& w,
                                         const KktIO& v) {
    const int N = a.N;
    double* ux = v.ux;
    double* pi = v.pi;
    double* lam = v.lam;
    double* t = v.t;
    const int l = lane_id();
    BoxCtx bc = box_ctx(w, v.d, lam, t);
    for (int i = l; i < (N + 1) * V16; i += 64) {
        ux[i] = w.ux_bkp[i];
        pi[i] = w.pi_bkp[i];
    }
    for (int i = l; i < (N + 1) * V32; i += 64) {
        t[i] = w.t_bkp[i];
        lam[i] = w.lam_bkp[i];
    }
    wsync();
    double mu = 0.0;
    ResIO ro{};
    ro.bsrc = v.vb + v.o16;
    ro.qsrc = v.vq + v.o16;
    if constexpr (NULLABLE) {
        if (!v.vb) ro.bsrc = nullptr;
        if (!v.vq) ro.qsrc = nullptr;
    }
    ro.ux = ux;
    ro.pi = pi;
    ro.rq = w.res_q;
    ro.rb = w.res_b;
    ro.rd = w.res_d;
    ro.rm = w.res_m;
    residual_pass<false, FX>(io, bc, ro, mu);
    wsync();
    HK_FOR_BOX(io, k, {
        w.qx[k * V16 + slot] = w.t_inv[lo] * (w.res_m[lo] - lam[lo] * w.res_d[lo]) -
                               w.t_inv[up] * (w.res_m[up] + lam[up] * w.res_d[up]);
    });
    HK_FOR_GEN(io, k, {
        w.qx[s16] = w.t_inv[lo] * (w.res_m[lo] - lam[lo] * w.res_d[lo]) -
                    w.t_inv[up] * (w.res_m[up] + lam[up] * w.res_d[up]);
    });
    wsync();
    double al = 1.0;
    ric_trs<BX_GIVEN, BX_NONE, FX>(io, sm, w.res_b, w.res_q, bc, w.dux, a.compute_mult, w.dpi, 1, w.Pb, al);
    wsync();
    HK_FOR_BOX(io, k, {  // d_compute_dt_dlam_res + d_update_var_res (alpha = 1)
        const int vi = bt.slotvar[k * 16 + slot];
        const double x = w.dux[k * V16 + vi];
        const double dtl = x - w.res_d[lo], dtu = -x + w.res_d[up];
        const double dll = -w.t_inv[lo] * (lam[lo] * dtl + w.res_m[lo]);
        const double dlu = -w.t_inv[up] * (lam[up] * dtu + w.res_m[up]);
        w.dt[lo] = dtl;
        w.dt[up] = dtu;
        w.dlam[lo] = dll;
        w.dlam[up] = dlu;
    });
    if (a.ngt) {  // the general slots: the same update from D dux (gen_alpha's phase-2 branch)
        for (int k = 0; k <= N; k++) {
            const StageInfo si = load_stage(io.st, k);
            if (si.ng == 0) continue;
            const DynSh sh(si);
            const int vc = tile_var(l & 15, sh.nu, sh.nx, sh.xo);
            double dummy = 1.0;
            gen_alpha<BX_P2>(io, sh, k, bc, gld(w.dux, k * V16 + vc, vc >= 0), dummy);
        }
    }
    wsync();
    for (int k = 0; k <= N; k++) {
        const StageInfo si = load_stage(io.st, k);
        if (l < si.nu + si.nx) ux[k * V16 + l] += 1.0 * w.dux[k * V16 + l];
        if (k < N && l < si.nx1) pi[k * V16 + l] += 1.0 * w.dpi[k * V16 + l];
    }
    HK_FOR_BOX(io, k, {
        lam[lo] += 1.0 * w.dlam[lo];
        lam[up] += 1.0 * w.dlam[up];
        t[lo] += 1.0 * w.dt[lo];
        t[up] += 1.0 * w.dt[up];
    });
    HK_FOR_GEN(io, k, {
        lam[lo] += 1.0 * w.dlam[lo];
        lam[up] += 1.0 * w.dlam[up];
        t[lo] += 1.0 * w.dt[lo];
        t[up] += 1.0 * w.dt[up];
    });
}

}  // namespace

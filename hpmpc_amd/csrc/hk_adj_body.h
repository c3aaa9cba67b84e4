// hk_adj_body.h -- the transpose of the KKT tangent solve (hk_tan_body.h), as a device function, one wavefront per call.
//
// The tangent T(db, dq, dd) -> (dux, dpi, dlam, dt) is, with w = lam_bkp * t_inv on every [lb | ub | lg | ug] slot and
// C the constraint rows (the selected variable of a box, D_k of a general constraint):
//   qx_j = -w_lo dd_lo - w_up dd_up;   (dux, dpi) = S(dq + C' qx, db);   dt_lo = C dux - dd_lo, dt_up = -C dux + dd_up,
//   dlam = -w dt,
// where S is ric_trs<BX_GIVEN, BX_NONE> on the persisted factor: minus the inverse of the symmetric KKT matrix, so
// S' = S under the pairing dux <-> dq, dpi <-> db.  For cotangents (gux, gpi, glam, gt) the transpose is therefore
//   h = gt - w glam on every slot, c_j = h_lo - h_up;   (y_ux, y_pi) = S(gux + C' c, gpi);
//   qbar = y_ux, bbar = y_pi, z = C y_ux, dbar_lo = -h_lo - w_lo z, dbar_up = h_up - w_up z:
// an element-wise pass, the tangent's ric_trs call (hq = gux, hb = gpi, bc.qx = c), an element-wise pass.
// Where the reference's x-pivot clamp fired on a stage (the P_eff record, hk_riccati.h) the persisted factor is not
// that of a symmetric system; the result is then DEFINED as these three steps, not as an exact transpose.
//
// Of the workspace the body READS F (through io.F), t_inv and lam_bkp, and never stores to it.  Every scratch element
// it reads it has written first: c over the box and general slots of qx, the zero res_d / res_m of the general slots
// (one vector serves both), h (kept in dbar's slots until dbar replaces it), z of the general slots (dt); Pb is
// written by the solve (compute_Pb = 1) and never read.
#pragma once
#include "hk_ipm_body.h"

namespace {

struct AdjIO {
    const double *gux, *gpi;         // cotangents of ux (variable order, V16) and pi (state order, V16): never null
    const double *glam, *gt;         // cotangents of lam and t (V32): null is zero
    double *qbar, *bbar, *dbar;      // the gradients (V16 / V16 / V32); dbar holds h between the passes
    double *qx, *Pb, *zero, *z, *zl; // work vectors of the set (V16 / V16 / V32 / V32 / V32)
    const double *t_inv, *lam_bkp;   // the workspace's (V32)
};

// `a`: N, ngt and compute_mult.  With compute_mult = 0, bbar is neither computed nor stored.  padded (wave-uniform):
// the gradients are the caller's padded arrays and every element of them is written (padding as zeros); otherwise
// only the elements the solve defines are (variables, multipliers of existing equations, existing constraint slots).
template <class FX>
__device__ __forceinline__ void adj_body(const KArgs& a, const RicIO& io, Scratch* sm, const BoxTab& bt,
                                         const AdjIO& v, bool padded) {
    const int N = a.N;
    const int l = lane_id();
    const double* lam = v.lam_bkp;
    if (padded) {
        for (int i = l; i < (N + 1) * V16; i += 64) {
            v.qbar[i] = 0.0;
            if (a.compute_mult) v.bbar[i] = 0.0;
        }
        for (int i = l; i < (N + 1) * V32; i += 64) v.dbar[i] = 0.0;
        wsync();
    }
    const auto cot = [&](const double* g, int i) { return g ? g[i] : 0.0; };
    // h = gt - w glam into dbar's slots, c = h_lo - h_up into qx
    HK_FOR_BOX(io, k, {
        const double hl = cot(v.gt, lo) - lam[lo] * v.t_inv[lo] * cot(v.glam, lo);
        const double hu = cot(v.gt, up) - lam[up] * v.t_inv[up] * cot(v.glam, up);
        v.dbar[lo] = hl;
        v.dbar[up] = hu;
        v.qx[k * V16 + slot] = hl - hu;
    });
    HK_FOR_GEN(io, k, {
        const double hl = cot(v.gt, lo) - lam[lo] * v.t_inv[lo] * cot(v.glam, lo);
        const double hu = cot(v.gt, up) - lam[up] * v.t_inv[up] * cot(v.glam, up);
        v.dbar[lo] = hl;
        v.dbar[up] = hu;
        v.qx[s16] = hl - hu;
        v.zero[lo] = 0.0;  // res_d and res_m of gen_alpha<BX_P2> below
        v.zero[up] = 0.0;
    });
    wsync();
    BoxCtx bc{};
    bc.Qx = v.qx;
    bc.qx = v.qx;
    // gen_alpha<BX_P2> with res_d = res_m = 0 stores dt_lo = D y_ux = z (and dt_up = -z, dlam: not used).  It also
    // loads t for a step-length candidate nobody uses; t_inv stands in so that the workspace's t_bkp is not touched
    bc.lam = const_cast<double*>(v.lam_bkp);
    bc.t = const_cast<double*>(v.t_inv);
    bc.t_inv = const_cast<double*>(v.t_inv);
    bc.res_d = v.zero;
    bc.res_m = v.zero;
    bc.dt = v.z;
    bc.dlam = v.zl;
    double al = 1.0;
    ric_trs<BX_GIVEN, BX_NONE, FX>(io, sm, v.gpi, v.gux, bc, v.qbar, a.compute_mult, v.bbar, 1, v.Pb, al);
    wsync();
    HK_FOR_BOX(io, k, {
        const int vi = bt.slotvar[k * 16 + slot];
        const double z = v.qbar[k * V16 + vi];
        const double hl = v.dbar[lo], hu = v.dbar[up];
        v.dbar[lo] = -hl - lam[lo] * v.t_inv[lo] * z;
        v.dbar[up] = hu - lam[up] * v.t_inv[up] * z;
    });
    if (a.ngt) {
        for (int k = 0; k <= N; k++) {
            const StageInfo si = load_stage(io.st, k);
            if (si.ng == 0) continue;
            const DynSh sh(si);
            const int vc = tile_var(l & 15, sh.nu, sh.nx, sh.xo);
            double dummy = 1.0;
            gen_alpha<BX_P2>(io, sh, k, bc, gld(v.qbar, k * V16 + vc, vc >= 0), dummy);
        }
        wsync();
        HK_FOR_GEN(io, k, {
            const double z = v.z[lo];
            const double hl = v.dbar[lo], hu = v.dbar[up];
            v.dbar[lo] = -hl - lam[lo] * v.t_inv[lo] * z;
            v.dbar[up] = hu - lam[up] * v.t_inv[up] * z;
        });
    }
}

}  // namespace

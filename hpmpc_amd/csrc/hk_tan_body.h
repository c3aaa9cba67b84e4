// hk_tan_body.h -- the linear part of d_kkt_solve_new_rhs_res_mpc_hard_tv (mpc_solvers/d_ip2_res_hard.c:1922-2299) in
// its right-hand sides, as a device function, one wavefront per call.  The re-solve (hk_kkt_body.h) is affine in
// (b, q, d): the factor is fixed, the step length is 1 and there is no line search (:2193-2237).  Its residuals
// (residual_pass, hk_ipm.h) carry b, q and d with unit coefficients -- r_q = q + .., r_b = b + .., r_d = d + .. on
// all four [lb | ub | lg | ug] slots -- and r_m = lam t does not depend on them.  So the tangent T(db, dq, dd) =
// kkt(b + db, q + dq, d + dd) - kkt(b, q, d) is the re-solve's Newton step with res_q = dq, res_b = db, res_d = dd
// and res_m = 0: no base solve, no subtraction, no residual pass, no backup copies; the step (dux, dpi, dlam, dt)
// is the result and nothing is added to it.
//
// Of the workspace the body READS F (through io.F), t_inv and lam_bkp, and never stores to it.  Every scratch element
// it reads (qx over the box and general slots, res_m over the general slots) it has written first; Pb is written by
// the solve (compute_Pb = 1) and never read.
#pragma once
#include "hk_ipm_body.h"

namespace {

struct TanIO {
    const double *hb, *hq, *rd;      // db (state order, V16), dq (variable order, V16), dd (V32): never null
    double *dux, *dpi, *dlam, *dt;   // the tangent (V16 / V16 / V32 / V32)
    double *qx, *Pb, *res_m;         // work vectors of the set (V16 / V16 / V32)
    const double *t_inv, *lam_bkp;   // the workspace's (V32)
};

// `a`: N, ngt and compute_mult.  With compute_mult = 0, dpi is returned as zeros.  padded (wave-uniform): the four
// results are the caller's padded arrays and every element of them is written (padding as zeros); otherwise only the
// elements the solve defines are (variables, multipliers of existing equations, existing constraint slots), plus
// the zero dpi.
template <class FX>
__device__ __forceinline__ void tan_body(const KArgs& a, const RicIO& io, Scratch* sm, const BoxTab& bt,
                                         const TanIO& v, bool padded) {
    const int N = a.N;
    const int l = lane_id();
    const double* lam = v.lam_bkp;
    if (padded || !a.compute_mult) {
        for (int i = l; i < (N + 1) * V16; i += 64) v.dpi[i] = 0.0;
    }
    if (padded) {
        for (int i = l; i < (N + 1) * V16; i += 64) v.dux[i] = 0.0;
        for (int i = l; i < (N + 1) * V32; i += 64) {
            v.dlam[i] = 0.0;
            v.dt[i] = 0.0;
        }
    }
    // the body's qx with res_m = 0
    HK_FOR_BOX(io, k, {
        v.qx[k * V16 + slot] = v.t_inv[lo] * (0.0 - lam[lo] * v.rd[lo]) - v.t_inv[up] * (0.0 + lam[up] * v.rd[up]);
    });
    HK_FOR_GEN(io, k, {
        v.qx[s16] = v.t_inv[lo] * (0.0 - lam[lo] * v.rd[lo]) - v.t_inv[up] * (0.0 + lam[up] * v.rd[up]);
        v.res_m[lo] = 0.0;  // read by gen_alpha<BX_P2> below
        v.res_m[up] = 0.0;
    });
    wsync();
    BoxCtx bc{};
    bc.Qx = v.qx;
    bc.qx = v.qx;
    // gen_alpha<BX_P2>: reads lam, t_inv, res_d, res_m, stores dt, dlam.  It also loads t for a step-length
    // candidate nobody uses; t_inv stands in so that the workspace's t_bkp is not touched
    bc.lam = const_cast<double*>(v.lam_bkp);
    bc.t = const_cast<double*>(v.t_inv);
    bc.t_inv = const_cast<double*>(v.t_inv);
    bc.res_d = const_cast<double*>(v.rd);
    bc.res_m = v.res_m;
    bc.dt = v.dt;
    bc.dlam = v.dlam;
    double al = 1.0;
    ric_trs<BX_GIVEN, BX_NONE, FX>(io, sm, v.hb, v.hq, bc, v.dux, a.compute_mult, v.dpi, 1, v.Pb, al);
    wsync();
    HK_FOR_BOX(io, k, {  // d_compute_dt_dlam_res with res_m = 0
        const int vi = bt.slotvar[k * 16 + slot];
        const double x = v.dux[k * V16 + vi];
        const double dtl = x - v.rd[lo], dtu = -x + v.rd[up];
        v.dt[lo] = dtl;
        v.dt[up] = dtu;
        v.dlam[lo] = -v.t_inv[lo] * (lam[lo] * dtl + 0.0);
        v.dlam[up] = -v.t_inv[up] * (lam[up] * dtu + 0.0);
    });
    if (a.ngt) {  // the general slots: the same from D dux (gen_alpha's phase-2 branch)
        for (int k = 0; k <= N; k++) {
            const StageInfo si = load_stage(io.st, k);
            if (si.ng == 0) continue;
            const DynSh sh(si);
            const int vc = tile_var(l & 15, sh.nu, sh.nx, sh.xo);
            double dummy = 1.0;
            gen_alpha<BX_P2>(io, sh, k, bc, gld(v.dux, k * V16 + vc, vc >= 0), dummy);
        }
    }
}

}  // namespace

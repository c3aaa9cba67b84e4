// hk_kkt.hip -- MI355X (gfx950): the batched KKT re-solve d_kkt_solve_new_rhs_res_mpc_hard_tv for device-resident
// batches, many right-hand-side sets per factor (hpmpc_mi355x_kkt_new_rhs_batch, hpmpc_mi355x_ocp_kkt_batch).
//
// One wavefront per (problem, right-hand-side set), grid = count * nrhs: workgroup j serves problem
// p = p0 + j / nrhs and set r = j % nrhs, set index s = p * nrhs + r.  The sets of one problem share its stage data
// and the workspace an IPM left (factor, t^-1, iterate backups), all read only; each set has its own b / q / d
// inputs, ux / pi / lam / t outputs and work vectors (a block of the caller's scratch), so the sets of a problem run
// at the same time and the workspace can be re-solved against again.  The arithmetic is hk_kkt_new_rhs's
// (hk_kkt_body.h), so a set's result does not depend on nrhs or on what else is in the launch.
#include "hk_kkt_args.h"
#include "hk_kkt_body.h"
#include "hk_kkt_launch.h"
#include "hk_launch.h"

template <class FX>
__global__ __launch_bounds__(64) void hk_kkt_rhs(KArgs a, KktArgs x) {
    const LdsTabs T = lds_tables(a);
    Scratch& sm = *T.sm;
    const int j = blockIdx.x;
    const int p = a.p0 + j / x.nrhs;
    if (p >= a.nprob) return;
    const long s = (long)p * x.nrhs + j % x.nrhs;
    const int N = a.N;
    Ws w = carve(a.ws + (long)p * a.sW, N);  // read only: F, t_inv and the backups
    // The ten work vectors: this set's scratch block.  This is carve_set (hk_kkt_args.h) written out: the kernel's
    // register allocation follows the form of these lines, and with them its code is the measured one.
    {
        const long n16 = (long)(N + 1) * V16, n32 = (long)(N + 1) * V32;
        double* S = x.scratch + s * x.sS;
        w.res_q = S;
        w.res_b = S + n16;
        w.qx = S + 2 * n16;
        w.dux = S + 3 * n16;
        w.dpi = S + 4 * n16;
        w.Pb = S + 5 * n16;
        S += KKT_SCRATCH_V16 * n16;
        w.res_d = S;
        w.res_m = S + n32;
        w.dt = S + 2 * n32;
        w.dlam = S + 3 * n32;
    }
    RicIO io = make_io(a, T, p, w.F);
    BoxTab bt{T.tileslot, T.slotvar};
    const long o16 = s * a.sV16, o32 = s * a.sV32;
    if (!a.compute_mult) {  // pi is not solved for: the body's pi = pi_bkp + dpi then returns the backup
        for (int i = lane_id(); i < (N + 1) * V16; i += 64) w.dpi[i] = 0.0;
    }
    const KktIO v{a.vb, a.vq, o16, a.d + o32, a.ux + o16, a.pi + o16, a.lam + o32, a.t + o32};
    kkt_body<FX, true>(a, io, &sm, bt, w, v);
}

extern "C" int hk_kkt_rhs_launch(const KArgs* a, const KktArgs* x, int count, hipStream_t stream) {
    return kkt_sets_launch(a, x, count, x->nrhs, stream,
                           [](auto fx) { return &hk_kkt_rhs<typename decltype(fx)::type>; });
}

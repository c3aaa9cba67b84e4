// hk_ocp_soft_args.h -- argument blocks of the soft OCP front end (hk_ocp_soft.hip), shared by the kernels and the
// host file hpmpc_capi_ocp_soft.cpp.  Plain C layout; every pointer is a device pointer.  Arrays are problem-major
// with the stride given next to them; a dense input with stride 0 is shared by every problem.
#pragma once
#include "hk_ocp_args.h"

// The twelve dense arrays (hpmpc_mi355x_ocp_soft_data in include/hpmpc_mi355x.h): the hard OCP's first ten at their
// HkOcpArray indices, so OcpStage's dense offsets serve them, then the slack penalties.  lb / ub hold nb + ns entries
// per stage (hard, then soft), Z / z hold 2 ns as [lower | upper].
enum HkOcpSoftArray { OCPS_Z = OCP_ub + 1, OCPS_z, OCPS_NARR };

// One stage: the hard OCP's table entry (o.nb / o.pnb: the HARD boxes; o.ng = 0; o.dn[OCP_lb] / [OCP_ub] count
// nb + ns per stage; lib4 blocks of the soft plan's tile plan) and the soft layout of hpmpc_mi355x_soft_offsets.
struct OcpSoftStage {
    OcpStage o;
    int ns, pns;
    int oD, oZ, oC;  // d_k (2 pnb + 2 pns), Z_k / z_k (2 pns), lam_k / t_k (2 pnb + 4 pns) inside one problem
    int dnZ;         // dense Z_k / z_k (2 ns) inside one problem
    int olam;        // the compact lam / t output (2 nb + 4 ns) inside one problem
    int pad;
};
static_assert(sizeof(OcpSoftStage) == 40 * sizeof(int), "OcpSoftStage is 40 ints");

struct OcpSoftPackArgs {
    int N, nprob, p0, count;
    int matrices;   // 0: only the b row of BAbt_k, the r / q row of RSQrq_k, d, Z, z (and ux) are rewritten
    int row_major;
    const OcpSoftStage* st;
    OcpIn in[OCPS_NARR];  // in[OCPS_z].p null: z packs as zeros
    double *BAbt, *RSQ;
    long long sB, sR;
    double *d, *Z, *z;  // packed, at oD / oZ
    long long sD, sZ;
    const double *u0, *x0;  // optional warm start, shaped like r / q
    long long su, sx;
    double* ux;  // V16 per stage, written only with u0 and x0
    long long sV16;
};

// hk_ocp_soft_res: d_res_mpc_soft_tv of one problem per workgroup.  res per problem: [r_q | r_b] 16 per stage, then
// r_d laid out like d, then r_z laid out like Z; mu per problem.
struct OcpSoftResArgs {
    int N, nprob, p0, count;
    const OcpSoftStage* st;
    const int* idxb;  // (N+1) * 16, hard then soft
    const double *BAbt, *RSQ, *d, *Z, *z, *ux, *pi, *lam, *t;
    long long sB, sR, sD, sZ, sC, sV16;
    double* res;
    long long sRes;
    double* mu;
};

// hk_ocp_soft_unpack: the iterate -> u, x, pi shaped like r, q, b and lam / t compact as [lo nb | up nb | 4 x ns];
// with `res` also the residual infinity norms.
struct OcpSoftUnpackArgs {
    int N, nprob, p0, count;
    const OcpSoftStage* st;
    const double *ux, *pi, *lam, *t;
    long long sV16, sC;
    OcpOut out;
    const double* res;  // hk_ocp_soft_res output; null: no norms
    long long sRes;
    const double* mu;
    double* inf;  // 4 per problem
};

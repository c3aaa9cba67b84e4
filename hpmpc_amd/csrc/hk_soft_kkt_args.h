// hk_soft_kkt_args.h -- argument blocks of the batched soft KKT re-solve (hk_soft_kkt.hip), shared by the kernels and
// the host file hpmpc_capi_soft_kkt.cpp.  Plain C layout; every pointer is a device pointer; offsets in doubles.
//
// hk_soft_kkt_factor / hk_soft_kkt_rhs take the tile kernels' KArgs for the problems (plan tables, BAbt / RSQ with the
// layout's strides, ws / sW: the soft IPM's workspaces) and for the right-hand-side sets: vb / vq the sets' b and q,
// ux / pi their outputs, sV16 between SETS; compute_mult.  Set s = p * nrhs + r belongs to problem p.  This block adds
// the soft layout, the constraint vectors and where the linearisation sits in a problem's workspace.
#pragma once
#include "hk_ocp_soft_args.h"
#include "hk_soft_args.h"
#include "hpmpc_kargs.h"

// Scratch of one set: qx (the box gradient, slot order) and Pb, V16 per stage each.  (N+1) * 32 doubles, a multiple
// of 256 bytes, so every set's vectors keep their cache-line alignment.
constexpr int SOFT_KKT_SCRATCH_V16 = 2;

inline long long soft_kkt_scratch_doubles(int N) { return (long long)(N + 1) * SOFT_KKT_SCRATCH_V16 * V16; }

struct SoftKktArgs {
    int nrhs;  // sets per problem: workgroup j serves problem p0 + j / nrhs, set j % nrhs
    int nq;    // ceil((N+1)/4) stage quads
    const SoftStage* st;
    const int* idxb;  // 16 per stage (hard then soft), shared by the batch
    // per problem, read only
    const double* Z;
    const double* z0;  // the problem's z: what a set takes when z is null
    long long sZ;
    const double *lam0, *t0;  // the base iterate of the factor launch
    long long sC;
    // per set, with the strides between sets
    const double *d, *z;  // z null: z0 of the set's problem
    long long sDs, sZs;
    double *lam, *t;
    long long sCs;
    // the linearisation inside a problem's workspace: lamt / tinv (laid out like lam), the flat Qx | qx | Zl | zl block
    // and the Riccati's Qx slots (V16 per stage).  The factor launch writes them, the set launch only reads lamt, tinv
    // and the Zl parts of the flat block
    long long oLamt, oTinv, oFlat, oVQx;
    double* scratch;  // nprob * nrhs blocks of sS doubles
    long long sS;
};

// hk_ocp_soft_kkt_pack: the dense vectors of count * nrhs sets -> the sets' blocks of the work buffer, b / [r | q]
// with 16 doubles per stage and d / z in the soft layouts (padding as zeros).  A set's block, sWk doubles:
//   [ b | q | ux | pi, (N+1) 16 each | d (sD) | z (sZ) | lam | t (sC each) ]
struct OcpSoftKktPackArgs {
    int N, nprob, p0, count, nrhs;
    const OcpSoftStage* st;
    const double *b, *q, *r, *lb, *ub, *z;  // (nprob, nrhs, size); z null: not packed
    long long nb_, nq_, nr_, nl_, nz_;       // their sizes per set
    double* work;
    long long sWk, oD, oZ;  // a set's stride, and where its d and z start
};

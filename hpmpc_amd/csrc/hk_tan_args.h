// hk_tan_args.h -- argument blocks of the batched KKT tangent solve and of the multi-set OCP finish (hk_tan.hip),
// shared by the kernels and the host file hpmpc_capi_tan.cpp.  Plain C layout; every pointer is a device pointer.
//
// hk_kkt_tan takes the tile kernels' KArgs exactly as hk_kkt_rhs does (hk_kkt_args.h): plan tables, BAbt / RSQ / DCt
// with the layout's strides, ws / sW (read only), and per direction set s = p * ndir + r the directions vb / vq / d
// (each nullable: a zero direction) and the outputs ux / pi / lam / t (dux, dpi, dlam, dt) with sV16 / sV32 between
// sets.  The set's scratch block is the re-solve's (kkt_scratch_doubles, the same carve).  With `ost` set (the OCP
// call) the directions are dense: the kernel's prologue seeds the scratch vectors from `in` and its epilogue writes
// the dense results; KArgs' per-set arrays are then not used.
#pragma once
#include <hip/hip_runtime.h>

#include "hk_kkt_args.h"
#include "hk_ocp_args.h"

struct TanArgs {
    int ndir;         // direction sets per problem: workgroup j serves problem p0 + j / ndir, set j % ndir
    double* scratch;  // nprob * ndir blocks of sS doubles
    long long sS;
    // dense mode (null ost: the padded arrays of KArgs)
    const OcpStage* ost;
    OcpIn in[OCP_NARR];               // only b, q, r, lb, ub, lg, ug are read; s: doubles between SETS; null: zero
    double *du, *dx, *dpo, *dlo, *dto;  // per set: shaped like r, q, b and compact [lb nb | ub nb | lg ng | ug ng]
    long long su, sx, sp, sl;
};

// hk_ocp_unpack_sets: hk_ocp_finish's data movement (equality-box fix included, no residuals) for nprob * nrhs sets
struct OcpSetsArgs {
    int N, nprob, p0, count, nrhs;
    const OcpStage* st;
    const int* idxb;  // (N+1) * 16
    const double *d, *ux, *pi, *lam, *t;  // padded, sV16 / sV32 between sets
    long long sV16, sV32;
    double *u, *x, *po, *lamo, *to;  // per set
    long long su, sx, sp, sl;
};

extern "C" {
// hk_tan.hip: a->ndir direction sets for each of `count` problems in one launch; the multi-set finish
int hk_kkt_tan_launch(const KArgs* a, const TanArgs* x, int count, hipStream_t stream);
int hk_ocp_unpack_sets_launch(const OcpSetsArgs* a, hipStream_t stream);
}

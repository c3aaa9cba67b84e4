// hk_matgrad_args.h -- argument block of the OCP matrix gradients (hk_ocp_matgrad, hk_matgrad.hip), shared by the
// kernel and the host file hpmpc_capi_kkt.cpp.  Plain C layout; every pointer is a device pointer.
//
// The base iterate (ux, pi, lam) is per problem in the padded layouts of the solver (sV16 / sV32 between problems);
// the adjoint solution (qbar, bbar, dbar) is per cotangent set s = p * nadj + r, padded likewise, with its own
// strides between sets: the caller's arrays (sV16 / sV32) or the dux / dpi / res_d vectors of the sets' scratch blocks
// (carve_set, hk_kkt_args.h; the scratch stride).  The gradients are dense, shaped like the data arrays.
#pragma once
#include "hk_adj_args.h"

struct MatGradArgs {
    int N, nprob, p0, count;
    int nadj;       // sets per problem: workgroup j serves set j / (N + 1) of the range, stage j % (N + 1)
    int row_major;  // the plan's storage order of a dense block
    const OcpStage* st;
    const double *ux, *pi, *lam;  // pi: null without A / B; lam: null without C / D or general constraints
    long long sV16, sV32;         // doubles between problems
    const double *qbar, *bbar, *dbar;  // bbar: null without A / B; dbar: as lam
    long long sq, sb, sd;              // doubles between sets
    OcpGrad grad;  // only the matrix entries A, B, Q, S, R, C, D are read; null: not wanted
};

// hk_matdir_args.h -- argument block of the OCP matrix directions (hk_ocp_matdir, hk_matdir.hip), shared by the kernel
// and the host file hpmpc_capi_kkt.cpp.  Plain C layout; every pointer is a device pointer.
//
// The base iterate (ux, pi, lam) is per problem in the padded layouts of the solver (sV16 / sV32 between problems);
// the directions are dense, shaped like the data arrays, per direction set s = p * ndir + r with dir[i].s doubles
// between sets; the seed rows (db, dq, dd) are per set, padded (16 / 16 / 32 doubles per stage), with their own strides
// between sets: the caller's arrays (sV16 / sV32) or the res_b / res_q / res_d vectors of the sets' scratch blocks
// (carve_set, hk_kkt_args.h; the scratch stride).
#pragma once
#include "hk_ocp_args.h"

struct MatDirArgs {
    int N, nprob, p0, count;
    int ndir;       // sets per problem: workgroup j serves set j / (N + 1) of the range, stage j % (N + 1)
    int row_major;  // the plan's storage order of a dense block
    const OcpStage* st;
    const double *ux, *pi, *lam;  // pi: null without A / B; lam: null without C / D or general constraints
    long long sV16, sV32;         // doubles between problems
    OcpIn dir[OCP_NARR];          // all fourteen are read; s: doubles between SETS; null: no term (matrix), zero (vector)
    double *db, *dq, *dd;         // the seed rows: every element of the sets in range is written
    long long sb, sq, sd;         // doubles between sets
};

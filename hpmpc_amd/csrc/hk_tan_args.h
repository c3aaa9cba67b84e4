// hk_tan_args.h -- argument block of the batched KKT tangent solve (hk_tan.hip), shared by the kernel and the host
// file hpmpc_capi_kkt.cpp.  Plain C layout; every pointer is a device pointer.
//
// hk_kkt_tan takes the tile kernels' KArgs exactly as hk_kkt_rhs does (hk_kkt_args.h): plan tables, BAbt / RSQ / DCt
// with the layout's strides, ws / sW (read only), and per direction set s = p * nrhs + r the directions vb / vq / d
// (each nullable: a zero direction) and the outputs ux / pi / lam / t (dux, dpi, dlam, dt) with sV16 / sV32 between
// sets.  The sets and their scratch blocks are the re-solve's (KktArgs: nrhs direction sets per problem, the same
// carve).  With `ost` set (the OCP call) the directions are dense: the kernel's prologue seeds the scratch vectors
// from `in` and its epilogue writes the dense results; KArgs' per-set arrays are then not used.
#pragma once
#include "hk_kkt_args.h"
#include "hk_ocp_args.h"

struct TanArgs {
    KktArgs k;
    // dense mode (null ost: the padded arrays of KArgs)
    const OcpStage* ost;
    OcpIn in[OCP_NARR];  // only b, q, r, lb, ub, lg, ug are read; s: doubles between SETS; null: zero
    OcpOut out;          // per set: du, dx, dpi, compact dlam, dt
};

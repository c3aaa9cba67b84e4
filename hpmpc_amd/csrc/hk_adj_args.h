// hk_adj_args.h -- argument block of the batched KKT adjoint solve (hk_adj.hip), shared by the kernel and the host
// file hpmpc_capi_kkt.cpp.  Plain C layout; every pointer is a device pointer.
//
// hk_kkt_adj takes the tile kernels' KArgs exactly as hk_kkt_tan does (hk_tan_args.h): plan tables, BAbt / RSQ / DCt
// with the layout's strides, ws / sW (read only), and per cotangent set s = p * nrhs + r the padded arrays with sV16 /
// sV32 between sets.  KArgs has the V16 ones and the one V32 output -- vq = gux, vb = gpi (each nullable: zero), ux =
// qbar, pi = bbar (null: not wanted, compute_mult = 0), lam = dbar -- and this block adds the two V32 cotangents KArgs
// has no read-only field for.  The sets and their scratch blocks are the re-solve's (KktArgs, the same carve).  With
// `ost` set (the OCP call) the cotangents and the gradients are dense: the kernel's prologue scatters `cot` into the
// scratch vectors and its epilogue gathers the dense gradients into `grad`; the per-set arrays are then not used.
#pragma once
#include "hk_kkt_args.h"
#include "hk_ocp_args.h"

// The dense gradients of one call: b, q, r, lb, ub, lg, ug shaped like the dense data arrays (HkOcpArray), s[i] doubles
// between sets; a null one is not wanted.
struct OcpGrad {
    double* p[OCP_NARR];
    long long s[OCP_NARR];
};

struct AdjArgs {
    KktArgs k;
    const double *glam, *gt;  // padded mode: V32 per stage, sV32 between sets; null: zero
    // dense mode (null ost: the padded arrays)
    const OcpStage* ost;
    OcpIn cot[5];  // gu, gx, gpi, compact glam, gt (the order of OcpOut); s: doubles between SETS; null: zero
    OcpGrad grad;
};

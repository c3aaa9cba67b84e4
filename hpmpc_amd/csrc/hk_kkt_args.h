// hk_kkt_args.h -- argument block of the batched KKT re-solve (hk_kkt.hip), shared by the kernel and the host file
// hpmpc_capi_kkt.cpp.  Plain C layout; every pointer is a device pointer.
//
// hk_kkt_rhs takes the tile kernels' KArgs for the problems (plan tables, BAbt / RSQ / DCt with the layout's strides,
// ws / sW: the workspaces an IPM left, read only) and for the right-hand-side sets: d, ux, pi, lam, t with sV16 /
// sV32 between SETS, vb / vq (nullable) the sets' b and q with sV16 between sets.  Set s = p * nrhs + r belongs to
// problem p.  This block adds what KArgs has no field for.
#pragma once
#include <hip/hip_runtime.h>

#include "hpmpc_kargs.h"

// Scratch of one set, in carve order: res_q, res_b, qx, dux, dpi, Pb (V16 per stage), then res_d, res_m, dt, dlam (V32
// per stage).  (N+1) * 224 doubles, a multiple of 256 bytes, so every set's vectors keep their cache-line alignment.
constexpr int KKT_SCRATCH_V16 = 6;
constexpr int KKT_SCRATCH_V32 = 4;

inline long long kkt_scratch_doubles(int N) {
    return (long long)(N + 1) * (KKT_SCRATCH_V16 * V16 + KKT_SCRATCH_V32 * V32);
}

struct KktArgs {
    int nrhs;         // sets per problem: workgroup j serves problem p0 + j / nrhs, set j % nrhs
    double* scratch;  // nprob * nrhs blocks of sS doubles
    long long sS;
};

// The ten work vectors of the set whose scratch block starts at S (hk_kkt_tan, hk_kkt_adj; hk_kkt_rhs writes the same
// lines out).
struct KktSet {
    double *res_q, *res_b, *qx, *dux, *dpi, *Pb, *res_d, *res_m, *dt, *dlam;
};
__host__ __device__ inline KktSet carve_set(double* S, int N) {
    const long long n16 = (long long)(N + 1) * V16, n32 = (long long)(N + 1) * V32;
    double* S32 = S + KKT_SCRATCH_V16 * n16;
    return {S, S + n16, S + 2 * n16, S + 3 * n16, S + 4 * n16, S + 5 * n16, S32, S32 + n32, S32 + 2 * n32, S32 + 3 * n32};
}

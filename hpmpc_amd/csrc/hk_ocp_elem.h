// hk_ocp_elem.h -- the element functions of the OCP front ends' pack kernels (hk_ocp_pack, hk_ocp.hip;
// hk_ocp_soft_pack, hk_ocp_soft.hip): the lib4 index of an output double, and the value of element (i, j) of BAbt_k /
// RSQrq_k gathered from the stage's dense blocks; and the wavefront maximum of their finish kernels.  Device code only.
#pragma once
#include "hk_ocp_args.h"

namespace {

// (row, column) of element e of a lib4 matrix with panel stride sd
__device__ __forceinline__ void lib4_rc(int e, int sd, int& i, int& j) {
    const int pw = 4 * sd, panel = e / pw, rem = e - panel * pw;
    i = 4 * panel + (rem & 3);
    j = rem >> 2;
}
__device__ __forceinline__ int lib4_at(int sd, int i, int j) { return (i >> 2) * 4 * sd + (i & 3) + 4 * j; }

// element (i, j) of a dense m x n block with leading sizes (m, n): column-major, or row-major
__device__ __forceinline__ double dense(const double* M, bool rm, int m, int n, int i, int j) {
    return M[rm ? i * n + j : i + j * m];
}

// BAbt_k = [B'; A'; b'], (nu + nx + 1) x nx1
__device__ __forceinline__ double babt_elem(const OcpStage& s, const double* A, const double* B, const double* b,
                                            bool rm, int i, int j) {
    if (j >= s.nx1) return 0.0;
    if (i < s.nu) return dense(B, rm, s.nx1, s.nu, j, i);
    const int ix = i - s.nu;
    if (ix < s.nx) return dense(A, rm, s.nx1, s.nx, j, ix);
    return ix == s.nx ? b[j] : 0.0;
}

// RSQrq_k = [[R S]; [S' Q]; [r' q']], (nu + nx + 1) x (nu + nx), both triangles
__device__ __forceinline__ double rsq_elem(const OcpStage& s, const double* Q, const double* S, const double* R,
                                           const double* q, const double* r, bool rm, int i, int j) {
    const int nu = s.nu, nux = s.nu + s.nx;
    if (j >= nux || i > nux) return 0.0;
    if (i == nux) return j < nu ? r[j] : q[j - nu];
    if (i < nu) return j < nu ? dense(R, rm, nu, nu, i, j) : dense(S, rm, nu, s.nx, i, j - nu);
    return j < nu ? dense(S, rm, nu, s.nx, j, i - nu) : dense(Q, rm, s.nx, s.nx, i - nu, j - nu);
}

__device__ __forceinline__ double wave_max(double v) {
#pragma unroll
    for (int m = 32; m >= 1; m >>= 1) v = fmax(v, __shfl_xor(v, m, 64));
    return v;
}

}  // namespace

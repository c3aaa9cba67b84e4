// hk_matdir.hip -- MI355X (gfx950): the OCP matrix directions (hpmpc_mi355x_ocp_matrix_dirs_batch,
// hpmpc_mi355x_ocp_tangent_data_batch).
//
// hk_ocp_matdir: the transposed twin of hk_ocp_matgrad (hk_matgrad.hip).  From a direction set in the dense data
// arrays (any of the fourteen) and the base iterate (ux = [u | x], pi, lam) of its problem, the seed row of the tangent
// solve: per stage k
//   db_k    = db + dA_k x_k + dB_k u_k
//   dr_k    = dr + sym(dR_k) u_k + dS_k x_k + dB_k' pi_k + dD_k' w_k
//   dq_k    = dq + sym(dQ_k) x_k + dS_k' u_k + dA_k' pi_k + dC_k' w_k
//   dd_lg,k = dlg - (dC_k x_k + dD_k u_k)      dd_ug,k = dug - (dC_k x_k + dD_k u_k)      dd_lb, dd_ub: the vectors'
// with w_k = lam_ug,k - lam_lg,k and sym(M) = (M + M') / 2: the residuals' dependence on the data at a fixed iterate
// (include/hpmpc_mi355x.h).  One workgroup of one wavefront per (stage, set), stage fastest, like hk_ocp_matgrad.  The
// stage's 64 base doubles go to LDS once; the GIVEN matrix blocks of the stage go to LDS in their storage order, laid
// end to end, lane t loading elements t, t + 64, .. (consecutive within a block: the hk_ocp_pack pattern), every load
// issued before the first LDS store.  Lane l then computes element l of the seed row in the placement of ocp_seed_bits
// (hk_ocp_place.h: lanes 0..15 db_k in state order, 16..31 [dr_k | dq_k], 32..63 dd_k) and stores it; every one of the
// 64 elements is written, padding as zeros, and nothing else is.
//
// Rounding.  An element starts from its vector direction (ocp_seed_bits; zero for a null vector).  Then every product
// of a GIVEN matrix is added with one fma each, in the order of the formulas above from left to right -- for db: A, B;
// for dr: R, S, B, D; for dq: Q, S, A, C -- and within a block by rising index of the summed dimension.  On the lg / ug
// slots the products of C, then D accumulate from zero in the same way and the sum is subtracted from the vector
// direction once.  A null matrix adds nothing, so without matrices the row is ocp_seed_bits' bit for bit; a set's row
// depends on nothing but its own directions and the base iterate; and every operation is exact under a common power of
// two, so scaling the directions by one scales the row bit for bit.
// Per stage and set up to nx1 (nu + nx) + (nu + nx)^2 + ng (nu + nx) direction doubles and 64 + 64 others are read for
// 64 written.  Measured at nprob 1024, N = 100, nx = 12, nu = 4 (448 direction doubles per stage and set), 1 / 4 sets
// per problem: 0.199 / 0.711 ms, 2.4 / 2.7 TB/s of those bytes -- the workgroup's serial chain (stage table -> loads ->
// LDS -> products -> store) counts as much as the bytes.  With one branch per kind of row element and loops of run-time
// length in place of the uniform runs below it took 0.231 / 0.843 ms.  64 threads, which hk_ocp_matgrad measured best;
// 128 were not tried.
#include <hip/hip_runtime.h>

#include "hk_launch.h"
#include "hk_launch_guard.h"
#include "hk_matdir_args.h"
#include "hk_ocp_place.h"

namespace {

constexpr int MD_THREADS = 64;
constexpr int MD_NMAT = 7;
// the stage's base iterate in LDS: [ux | pi] V16 each, then lam V32
constexpr int MD_UX = 0, MD_PI = V16, MD_LAM = 2 * V16, MD_BASE = 2 * V16 + V32;
// the direction blocks: [A | B] has nx1 <= V16 rows of nu + nx <= V16 columns, Q, S, R fit the (nu + nx)^2 square and
// [C | D] has ng <= V16 rows (d_k is one V32 vector), so a stage's blocks are at most three V16 x V16 squares
constexpr int MD_DIR = 3 * V16 * V16;
constexpr int MD_LOADS = MD_DIR / MD_THREADS;
enum { M_A, M_B, M_Q, M_S, M_R, M_C, M_D };

}  // namespace

__global__ __launch_bounds__(MD_THREADS) void hk_ocp_matdir(MatDirArgs a) {
    __shared__ double base[MD_BASE];
    __shared__ double blk[MD_DIR];
    const unsigned n1 = a.N + 1;
    const int k = blockIdx.x % n1;
    const unsigned j = blockIdx.x / n1;
    const unsigned pj = j / (unsigned)a.ndir;
    if (pj >= (unsigned)a.count) return;
    const long p = (long)a.p0 + pj;
    if (p >= a.nprob) return;
    const long s = p * a.ndir + j % (unsigned)a.ndir;
    const OcpStage st = a.st[k];
    const int l = threadIdx.x;
    // the given blocks of the stage, end to end, in the arrays' order
    constexpr int key[MD_NMAT] = {OCP_A, OCP_B, OCP_Q, OCP_S, OCP_R, OCP_C, OCP_D};
    const int rows[MD_NMAT] = {st.nx1, st.nx1, st.nx, st.nu, st.nu, st.ng, st.ng};
    const int cols[MD_NMAT] = {st.nx, st.nu, st.nx, st.nx, st.nu, st.nx, st.nu};
    int cum[MD_NMAT + 1];
    const double* inp[MD_NMAT];
    bool has[MD_NMAT];
    cum[0] = 0;
#pragma unroll
    for (int i = 0; i < MD_NMAT; i++) {
        const double* d = a.dir[key[i]].p;
        has[i] = d != nullptr;
        cum[i + 1] = cum[i] + (d ? rows[i] * cols[i] : 0);
        inp[i] = d ? d + s * a.dir[key[i]].s + st.dn[key[i]] : nullptr;
    }
    const int total = cum[MD_NMAT] < MD_DIR ? cum[MD_NMAT] : MD_DIR;  // never more: the sizes above
    // ---- loads: the vector directions' element, the base iterate's, the blocks' -- all issued before the first store
    const auto in = [&](int i) -> const double* { return a.dir[i].p ? a.dir[i].p + s * a.dir[i].s : nullptr; };
    const OcpVecs vec{in(OCP_b), in(OCP_q), in(OCP_r), in(OCP_lb), in(OCP_ub), in(OCP_lg), in(OCP_ug)};
    const long long seed = ocp_seed_bits(st, vec, l);
    const long o16 = p * a.sV16 + (long)k * V16, o32 = p * a.sV32 + (long)k * V32;
    const double* bsrc = l < MD_PI    ? a.ux + o16 + l
                         : l < MD_LAM ? (a.pi ? a.pi + o16 + (l - MD_PI) : nullptr)
                                      : (a.lam ? a.lam + o32 + (l - MD_LAM) : nullptr);
    const double bval = bsrc ? *bsrc : 0.0;
    double v[MD_LOADS];
#pragma unroll
    for (int i = 0; i < MD_LOADS; i++) {
        const int e = l + i * MD_THREADS;
        // the block of element e: the last one that starts at or before it (an empty block is passed over)
        const double* src = inp[0];
        int start = 0;
#pragma unroll
        for (int m = 1; m < MD_NMAT; m++) {
            if (e >= cum[m]) {
                src = inp[m];
                start = cum[m];
            }
        }
        v[i] = e < total ? src[e - start] : 0.0;
    }
    base[l] = bval;
#pragma unroll
    for (int i = 0; i < MD_LOADS; i++) {
        const int e = l + i * MD_THREADS;
        if (e < total) blk[e] = v[i];
    }
    __syncthreads();
    const double *ux = base + MD_UX, *pi = base + MD_PI, *lam = base + MD_LAM;
    const bool rm = a.row_major != 0;
    // Lane l's role: row i of db_k (ROLE_B), input i of dr_k (ROLE_U), state i of dq_k (ROLE_X), general constraint i of
    // dd_k's lower or upper side (ROLE_D), or padding.  Every role is a chain of at most four terms, each a run along a
    // row or a column of one block against a vector of the base iterate:
    //           term 0           term 1          term 2 (pi)     term 3 (w)
    //   ROLE_B  A[i, :] x        B[i, :] u
    //   ROLE_U  sym(R)[i, :] u   S[i, :] x       B[:, i]' pi     D[:, i]' w
    //   ROLE_X  sym(Q)[i, :] x   S[:, i]' u      A[:, i]' pi     C[:, i]' w
    //   ROLE_D  C[i, :] x        D[i, :] u       (accumulated from zero and subtracted from the vector direction once)
    // The four roles run the same code with their own addresses and counts, so the wavefront does not serialise them,
    // and the trip counts are wave-uniform and unrolled by four, so the LDS reads of four products are in flight
    // together; a lane past its own count reads element 0 and keeps its sum.
    enum { ROLE_B, ROLE_U, ROLE_X, ROLE_D, ROLE_NONE };
    const int iu = ocp_u_of_slot(st, l - V16), ix = ocp_x_of_slot(st, l - V16);
    const int lo = ocp_lg_of_slot(st, l - 2 * V16), up = ocp_ug_of_slot(st, l - 2 * V16);
    const int role = l < st.nx1 ? ROLE_B : iu >= 0 ? ROLE_U : ix >= 0 ? ROLE_X : (lo >= 0 || up >= 0) ? ROLE_D : ROLE_NONE;
    const int i = role == ROLE_B ? l : role == ROLE_U ? iu : role == ROLE_X ? ix : role == ROLE_D ? (lo >= 0 ? lo : up) : 0;
    struct Run {
        int a0, as, cnt;  // element c of the run is blk[a0 + c * as], c < cnt
    };
    // row i / column i of given block m in the plan's storage order; a null block or an idle lane has no element
    const auto row = [&](int m, bool on) -> Run {
        return {cum[m] + (rm ? i * cols[m] : i), rm ? 1 : rows[m], on && has[m] ? cols[m] : 0};
    };
    const auto col = [&](int m, bool on) -> Run {
        return {cum[m] + (rm ? i : i * rows[m]), rm ? cols[m] : 1, on && has[m] ? rows[m] : 0};
    };
    const auto pick = [](bool c, const Run& x, const Run& y) -> Run { return c ? x : y; };
    const bool isb = role == ROLE_B, isu = role == ROLE_U, isx = role == ROLE_X, isd = role == ROLE_D;
    const Run none{0, 0, 0};
    const Run t0 = pick(isb, row(M_A, true), pick(isu, row(M_R, true), pick(isx, row(M_Q, true), row(M_C, isd))));
    const Run t0s = pick(isu, col(M_R, true), pick(isx, col(M_Q, true), t0));  // sym: the transposed element
    const Run t1 = pick(isb, row(M_B, true), pick(isu, row(M_S, true), pick(isx, col(M_S, true), row(M_D, isd))));
    const Run t2 = pick(isu, col(M_B, true), pick(isx, col(M_A, true), none));
    const Run t3 = pick(isu, col(M_D, true), pick(isx, col(M_C, true), none));
    const bool sym0 = isu || isx, x0 = !isu, x1 = isu;  // term 0 / 1 run against x (else u)
    const double seedv = __longlong_as_double(seed);
    double acc = isd ? 0.0 : seedv;
    const int nux = st.nx > st.nu ? st.nx : st.nu;
    if (has[M_A] || has[M_R] || has[M_Q] || has[M_C]) {
        for (int c0 = 0; c0 < nux; c0 += 4) {
#pragma unroll
            for (int c = c0; c < c0 + 4; c++) {
                const bool ok = c < t0.cnt;
                const int cc = ok ? c : 0;
                const double e = blk[t0.a0 + cc * t0.as], f = blk[t0s.a0 + cc * t0s.as];
                const double x = ux[x0 ? ocp_slot_x(st, cc) : ocp_slot_u(st, cc)];
                const double sum = fma(sym0 ? 0.5 * (e + f) : e, x, acc);
                acc = ok ? sum : acc;
            }
        }
    }
    if (has[M_B] || has[M_S] || has[M_D]) {
        for (int c0 = 0; c0 < nux; c0 += 4) {
#pragma unroll
            for (int c = c0; c < c0 + 4; c++) {
                const bool ok = c < t1.cnt;
                const int cc = ok ? c : 0;
                const double sum = fma(blk[t1.a0 + cc * t1.as], ux[x1 ? ocp_slot_x(st, cc) : ocp_slot_u(st, cc)], acc);
                acc = ok ? sum : acc;
            }
        }
    }
    if (has[M_A] || has[M_B]) {
        for (int c0 = 0; c0 < st.nx1; c0 += 4) {
#pragma unroll
            for (int c = c0; c < c0 + 4; c++) {
                const bool ok = c < t2.cnt;
                const int cc = ok ? c : 0;
                const double sum = fma(blk[t2.a0 + cc * t2.as], pi[cc], acc);
                acc = ok ? sum : acc;
            }
        }
    }
    if (has[M_C] || has[M_D]) {
        for (int c0 = 0; c0 < st.ng; c0 += 4) {
#pragma unroll
            for (int c = c0; c < c0 + 4; c++) {
                const bool ok = c < t3.cnt;
                const int cc = ok ? c : 0;
                const double w = lam[ocp_slot_ug(st, cc)] - lam[ocp_slot_lg(st, cc)];
                const double sum = fma(blk[t3.a0 + cc * t3.as], w, acc);
                acc = ok ? sum : acc;
            }
        }
    }
    const double r = !isd ? acc : (has[M_C] || has[M_D]) ? seedv - acc : seedv;
    double* dst = l < V16       ? a.db + s * a.sb + (long)k * V16 + l
                  : l < 2 * V16 ? a.dq + s * a.sq + (long)k * V16 + (l - V16)
                                : a.dd + s * a.sd + (long)k * V32 + (l - 2 * V16);
    *dst = r;
}

extern "C" int hk_ocp_matdir_launch(const MatDirArgs* a, hipStream_t stream) {
    if (a->count <= 0 || a->ndir <= 0) return 0;
    static const HkKernelLimits lim(reinterpret_cast<const void*>(&hk_ocp_matdir));
    if (const int e = lim.check(0, MD_THREADS)) return e;
    const long long blocks = (long long)a->count * a->ndir * (a->N + 1);
    if (blocks > 0x7fffffffLL) return HK_LAUNCH_REFUSED;
    hipLaunchKernelGGL(hk_ocp_matdir, dim3((unsigned)blocks), dim3(MD_THREADS), 0, stream, *a);
    return (int)hipGetLastError();
}

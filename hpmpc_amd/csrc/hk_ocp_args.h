// hk_ocp_args.h -- argument blocks of the batched OCP front end (hk_ocp.hip), shared by the kernels and the host
// file hpmpc_capi_ocp.cpp.  Plain C layout; every pointer is a device pointer.  Arrays are problem-major with the
// stride given next to them; a dense input with stride 0 is shared by every problem.
#pragma once

// The fourteen dense arrays, in the order of the c_interface.h wrappers' argument lists (and of
// hpmpc_mi355x_ocp_data in include/hpmpc_mi355x.h).  The order groups them by the packed block they feed -- the
// sections of hk_ocp_pack: A B b -> BAbt_k | Q S R q r -> RSQrq_k | lb ub C D lg ug -> d_k and DCt_k.
enum HkOcpArray {
    OCP_A, OCP_B, OCP_b, OCP_Q, OCP_S, OCP_R, OCP_q, OCP_r, OCP_lb, OCP_ub, OCP_C, OCP_D, OCP_lg, OCP_ug, OCP_NARR
};
enum HkOcpSection { OCP_SEC_BABT, OCP_SEC_RSQ, OCP_SEC_DCT, OCP_NSEC };

// One stage: sizes, the lib4 blocks of the tile plan's packed default layout, and the offsets (doubles) of the
// stage's block inside one problem of every dense array.  The u / x / pi outputs sit at dn[OCP_r] / dn[OCP_q] /
// dn[OCP_b] (the arrays have the shapes of r / q / b), the lam / t outputs at 2 dn[OCP_lb] + 2 dn[OCP_lg].
struct OcpStage {
    int nu, nx, nx1, nb, ng, pnb, png;
    int nbu;           // leading boxes that sit on inputs (the equality-box fix's loop bound); 0 on stage N
    int sd[OCP_NSEC];  // panel stride of BAbt_k, RSQrq_k, DCt_k
    int n[OCP_NSEC];   // doubles of the three lib4 blocks (0: the stage has none)
    int o[OCP_NSEC];   // their offsets inside one problem
    int dn[OCP_NARR];  // dense offsets, by HkOcpArray
    int pad;
};
static_assert(sizeof(OcpStage) == 32 * sizeof(int), "OcpStage is 32 ints");

struct OcpIn {
    const double* p;
    long long s;  // doubles between problems (0: shared)
};

struct OcpPackArgs {
    int N, nprob, p0, count;
    int matrices;   // 0: only the b row of BAbt_k, the r / q row of RSQrq_k and d are rewritten
    int row_major;  // the c_order_ convention; 0: column-major blocks (fortran_order_)
    const OcpStage* st;
    OcpIn in[OCP_NARR];
    double* out[OCP_NSEC];  // BAbt, RSQrq, DCt
    long long sout[OCP_NSEC];
    double* d;
    long long sV32;
    const double *u0, *x0;  // optional warm start, shaped like r / q
    long long su, sx;
    double* ux;  // V16 per stage, written only with u0 and x0
    long long sV16;
};

// The dense outputs: u, x, pi shaped like r, q, b, lam / t compact [lb nb | ub nb | lg ng | ug ng] per stage, with the
// doubles between problems (or sets).  t is nullable.  Filled from the plan by ocp_out (hk_ocp_plan.h).
struct OcpOut {
    double *u, *x, *pi, *lam, *t;
    long long su, sx, sp, sl;
};

// hk_ocp_unpack: the padded iterate of nprob * nsets sets -> the dense outputs (set s = p * nsets + r; sV16 / sV32
// and the output strides are between sets).  With `res` (hpmpc_mi355x_ocp_finish_batch; nsets = 1) also the
// residual infinity norms.
struct OcpUnpackArgs {
    int N, nprob, p0, count, nsets;
    const OcpStage* st;
    const int* idxb;  // (N+1) * 16
    const double *d, *ux, *pi, *lam, *t;
    long long sV16, sV32;
    OcpOut out;
    const double* res;  // hk_res output per problem: [rq | rb] V16 per stage, [rd | rm] V32 per stage; null: no norms
    long long sRes;
    const double* mu;  // per problem
    double* inf;       // 4 per problem
};

// hk_ocp_plan.h -- the OCP plan of the batched OCP front end, shared by hpmpc_capi_ocp.cpp (which creates it) and
// hpmpc_capi_kkt.cpp (the dense tangent and adjoint calls): a tile plan, whose packed default layout the lib4
// and vector arrays follow, and the device tables of stage sizes, dense offsets (OcpStage, hk_ocp_args.h) and box
// indices.
#pragma once
#include <memory>

#include "hk_ocp_args.h"
#include "hk_plan.h"

struct hpmpc_mi355x_ocp_plan {
    std::unique_ptr<hpmpc_mi355x_plan> tile;
    int N = 0, row_major = 0;
    std::vector<OcpStage> st;
    long long dense[OCP_NARR] = {};  // doubles per problem of every dense array
    long long su = 0, sx = 0, sp = 0, sl = 0;  // u, x, pi, lam / t outputs
    long long sRes = 0;                        // hk_res output per problem
    DevTable<OcpStage> d_st;
    DevTable<int> d_idx;
};

// The dense outputs of a call on plan O, and whether every one the plan has an element of is given (t: when asked).
inline OcpOut ocp_out(const hpmpc_mi355x_ocp_plan* O, double* u, double* x, double* pi, double* lam, double* t) {
    return {u, x, pi, lam, t, O->su, O->sx, O->sp, O->sl};
}
inline bool ocp_out_ok(const OcpOut& o, bool need_t) {
    return (o.su == 0 || o.u) && (o.sx == 0 || o.x) && (o.sp == 0 || o.pi) && (o.sl == 0 || (o.lam && (o.t || !need_t)));
}

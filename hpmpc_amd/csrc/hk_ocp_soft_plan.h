// hk_ocp_soft_plan.h -- the soft OCP plan of the soft OCP front end, shared by hpmpc_capi_ocp_soft.cpp (which creates
// it, packs, solves and finishes on it) and hpmpc_capi_soft_kkt.cpp (the soft KKT re-solve on dense per-set vectors).
#pragma once
#include "hk_ocp_soft_args.h"
#include "hk_soft_plan.h"

struct hpmpc_mi355x_ocp_soft_plan {
    std::unique_ptr<hpmpc_mi355x_soft_plan> soft;
    int N = 0, row_major = 0, res_ok = 0;
    std::vector<OcpSoftStage> st;
    long long dense[OCPS_NARR] = {};           // doubles per problem of every dense array
    long long su = 0, sx = 0, sp = 0, sl = 0;  // u, x, pi, lam / t outputs
    long long sRes = 0;                        // hk_ocp_soft_res output per problem
    DevTable<OcpSoftStage> d_st;
};

namespace {

inline OcpOut soft_out(const hpmpc_mi355x_ocp_soft_plan* O, double* u, double* x, double* pi, double* lam, double* t) {
    return {u, x, pi, lam, t, O->su, O->sx, O->sp, O->sl};
}
inline bool soft_out_ok(const OcpOut& o) {
    return (o.su == 0 || o.u) && (o.sx == 0 || o.x) && (o.sp == 0 || o.pi) && (o.sl == 0 || o.lam);
}

}  // namespace

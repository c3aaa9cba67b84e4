// hk_soft_plan.h -- the soft plan of the batched soft-constraint IPM, shared by hpmpc_capi_soft_batch.cpp (which
// creates it and solves on it), hpmpc_capi_soft_kkt.cpp (the soft KKT re-solve, which reads the workspace carve) and
// hpmpc_capi_ocp_soft.cpp (the soft OCP front end, whose plan owns one, through hk_ocp_soft_plan.h): a tile plan
// on nb + ns boxes per stage, the soft layout and the workspace carve.
#pragma once
#include <memory>

#include "hk_plan.h"

struct hpmpc_mi355x_soft_plan {
    std::unique_ptr<hpmpc_mi355x_plan> tile;
    int N = 0;
    SoftLayout L;
    double mu_scal = 0.0;  // soft_mu_scal; 0: no constraint anywhere
    // workspace carve (doubles)
    long long oV16 = 0, oCv = 0, nCv = 0, oFlat = 0, oScal = 0, oIst = 0, ws = 0;
    DevTable<SoftStage> d_st;
    DevTable<int> d_idx;
};

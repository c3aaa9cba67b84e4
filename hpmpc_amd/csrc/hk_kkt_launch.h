// hk_kkt_launch.h -- the launcher of the one-wavefront-per-set kernels hk_kkt_rhs (hk_kkt.hip), hk_kkt_tan
// (hk_tan.hip) and hk_kkt_adj (hk_adj.hip): grid = count problems x `sets` sets per problem, the LDS stage tables, the launch guard.
#pragma once
#include "hk_ipm_body.h"
#include "hk_launch_guard.h"

// kernel_of(FxTag<FX>{}): the kernel's instantiation for the compiled inner-stage class FX, the tile plan's
// (KArgs.fixcls), as in hk_launch.  Every call site passes its own lambda, so `lim` is one object per kernel.
template <class X, class KernelOf>
static int kkt_sets_launch(const KArgs* a, const X* x, int count, int sets, hipStream_t stream, KernelOf kernel_of) {
    if (count <= 0 || sets <= 0) return 0;
    return with_fixcls(a->fixcls, [&](auto fx) {
        const auto kernel = kernel_of(fx);
        // the launch guard (hk_launch_guard.h): LDS tables, private segment against the stack limit, launch bound
        static const HkKernelLimits lim(reinterpret_cast<const void*>(kernel));
        const size_t lds = lds_table_bytes(a->N);
        if (const int e = lim.check(lds, 64)) return e;
        hipLaunchKernelGGL(kernel, dim3((unsigned)count * (unsigned)sets), dim3(64), lds, stream, *a, *x);
        return (int)hipGetLastError();
    });
}

// hk_launch.h -- the launch functions the kernel translation units (*.hip) define and the host C-ABI files call.
// extern "C" names are not mangled, so a prototype repeated by hand at a call site would still link after its
// signature drifted; every definer and every caller includes this header instead, and a mismatch is a compile
// error.  The launch ids (`which`) are the enums next to each argument block (hpmpc_kargs.h, hk_soft_args.h,
// hk_wide_args.h).  Return: 0, a hipError_t, -1 for an unknown id, or HK_LAUNCH_REFUSED (hk_launch_guard.h).
#pragma once
#include <hip/hip_runtime.h>

struct KArgs;
struct KktArgs;
struct SoftArgs;
struct SoftResArgs;
struct WideIpmArgs;
struct TanArgs;
struct AdjArgs;
struct MatGradArgs;
struct MatDirArgs;
struct OcpPackArgs;
struct OcpUnpackArgs;
struct OcpSoftPackArgs;
struct OcpSoftResArgs;
struct OcpSoftUnpackArgs;
struct SoftKktArgs;
struct OcpSoftKktPackArgs;

extern "C" {
// hpmpc_kernels.hip: the tile kernels (which: HkLaunch) and the compiled inner-stage class of a stage size
int hk_launch(int which, const KArgs* a, int count, hipStream_t stream);
int hk_fixcls(int nu, int nx);
#ifdef HK_RIC2  // the two-wave sv (hk_ric2.hip), a measured negative result: only in the ric2 build variant
int hk_launch_ric2(int which, const KArgs* a, int count, hipStream_t stream);
#endif
// hk_soft.hip: the soft-constraint IPM passes (which: HkSoftPass) and the soft residual
int hk_soft_launch(int which, const SoftArgs* a, int count, hipStream_t stream);
int hk_soft_res_launch(const SoftResArgs* a, hipStream_t stream);
// hk_soft_ipm.hip: the batched soft-constraint IPM, init launch + one launch for every iteration of every problem
int hk_soft_ipm_launch(const KArgs* a, const SoftArgs* s, int count, hipStream_t stream);
// hk_kkt.hip: the batched KKT re-solve, x->nrhs right-hand-side sets for each of `count` problems in one launch
int hk_kkt_rhs_launch(const KArgs* a, const KktArgs* x, int count, hipStream_t stream);
// hk_tan.hip: the batched KKT tangent solve, x->k.nrhs direction sets for each of `count` problems in one launch
int hk_kkt_tan_launch(const KArgs* a, const TanArgs* x, int count, hipStream_t stream);
// the same in dense mode with the prologue skipped: the sets' scratch blocks already hold the seed rows (hk_ocp_matdir)
int hk_kkt_tan_seeded_launch(const KArgs* a, const TanArgs* x, int count, hipStream_t stream);
// hk_adj.hip: the batched KKT adjoint solve, x->k.nrhs cotangent sets for each of `count` problems in one launch
int hk_kkt_adj_launch(const KArgs* a, const AdjArgs* x, int count, hipStream_t stream);
// hk_matgrad.hip: the OCP matrix gradients, one workgroup per (stage, set) of a->count * a->nadj sets in one launch
int hk_ocp_matgrad_launch(const MatGradArgs* a, hipStream_t stream);
// hk_matdir.hip: the OCP matrix directions, one workgroup per (stage, set) of a->count * a->ndir sets in one launch
int hk_ocp_matdir_launch(const MatDirArgs* a, hipStream_t stream);
// hk_wide.hip (which: HkWideLaunch; args: the WideArgs / PcArgs / PxArgs of that kernel) and hk_wide_ipm.hip
int hk_wide_launch(int which, const void* args, int count, int lds_doubles, hipStream_t stream);
int hk_wide_ipm_launch(const WideIpmArgs* a, int count, int lds_doubles, hipStream_t stream);
// hk_ocp.hip: the batched OCP front end, dense data -> lib4 (grid: stages x a->count problems) and the iterates of
// a->count * a->nsets sets -> outputs (with a->res: the finish, one set per problem and the residual norms)
int hk_ocp_pack_launch(const OcpPackArgs* a, hipStream_t stream);
int hk_ocp_unpack_launch(const OcpUnpackArgs* a, hipStream_t stream);
// hk_ocp_soft.hip: the soft OCP front end, dense data -> lib4 and the soft layouts (a->matrices: the matrix sections
// and the vectors, two launches; else the vectors alone), the batched d_res_mpc_soft_tv (one workgroup per problem)
// and the iterates -> outputs (with a->res: the residual norms)
int hk_ocp_soft_pack_launch(const OcpSoftPackArgs* a, hipStream_t stream);
int hk_ocp_soft_res_launch(const OcpSoftResArgs* a, hipStream_t stream);
int hk_ocp_soft_unpack_launch(const OcpSoftUnpackArgs* a, hipStream_t stream);
// hk_soft_kkt.hip: the batched soft KKT re-solve, with `refactor` the factor launch (one wavefront per problem), then
// x->nrhs right-hand-side sets for each of `count` problems in one launch; and the dense vectors of a->count * a->nrhs
// sets -> their padded vectors
int hk_soft_kkt_launch(const KArgs* a, const SoftKktArgs* x, int count, int refactor, hipStream_t stream);
int hk_ocp_soft_kkt_pack_launch(const OcpSoftKktPackArgs* a, hipStream_t stream);
}

// hk_host.h -- what every host translation unit of libhpmpc_mi355x.so (hpmpc_capi*.cpp) shares: the lib4
// constants and index helpers, the thread's error code, the one thread-local device context of the host-buffer
// entry points, and the single declaration of every function one hpmpc_capi*.cpp defines for another (the kernel
// launchers are in hk_launch.h).  The files that define these functions include this header too, so a signature
// that drifts on one side is a compile error instead of garbage pointers handed to a kernel.
#pragma once
#include <hip/hip_runtime.h>

#include <cstdio>
#include <cstring>
#include <vector>

#include "hpmpc_api.h"
#include "hk_launch.h"

// Error code of the calling thread's last API call (hpmpc_mi355x_last_error); defined in hpmpc_capi.cpp.
extern thread_local int g_err;

extern "C" {
// hpmpc_capi.cpp: records the code and, when it is nonzero, prints one stderr line; code 0 clears the error
void hk_set_error(int code, const char* what);
// hpmpc_capi_wide.cpp: the drop-in Riccati entry points on stages beyond the 16-wide tile (partial condensing on the
// same stages is hpmpc_capi_pcond.cpp; its entry points are public, include/hpmpc_mi355x.h)
long long hk_wide_factor_bytes(int N, const int* nx, const int* nu);
void hk_wide_sv_entry(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, int update_b, double** hpBAbt,
                      double** b, int update_q, double** hpQ, double** q, double** bd, double** hpDCt, double** Qx,
                      double** qx, double** hux, int compute_pi, double** hpi, int compute_Pb, double** hPb,
                      double* memory);
void hk_wide_trf_entry(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt, double** hpQ,
                       double** hpDCt, double** Qx, double** bd, double* memory);
void hk_wide_trs_entry(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt, double** hb,
                       double** hq, double** hpDCt, double** qx, double** hux, int compute_pi, double** hpi,
                       int compute_Pb, double** hPb, double* memory);
// hpmpc_capi_wide_ipm.cpp: the drop-in IPM, KKT re-solve and residual entry points on the same stages
// (mode: WI_*, hk_wide_args.h)
long long hk_wide_ipm_bytes(int N, const int* nx, const int* nu, const int* nb, const int* ng);
int hk_wide_ipm_entry(int mode, int* kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                      double* stat, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng, double** pBAbt,
                      double** pQ, double** pDCt, double** d, double** ux, int compute_mult, double** pi,
                      double** lam, double** t, double* work, double** ux0, double** pi0, double** lam0, double** t0);
void hk_wide_kkt_entry(int p1, int N, int* nx, int* nu_N, int* nb, int** idxb, int* ng, double** pBAbt, double** b,
                       double** pQ, double** q, double** pDCt, double** d, double** ux, int compute_mult, double** pi,
                       double** lam, double** t, double* work);
void hk_wide_res_entry(int plain, int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                       double** hb, double** hpQ, double** hq, double** hux, double** hpDCt, double** hd,
                       double** hpi, double** hlam, double** ht, double** hrq, double** hrb, double** hrd,
                       double** hrm, double* mu);
}

constexpr int BS = 4, NCL = 2;  // lib4: panel height, column-count granule of the panel stride

inline int rup(int n, int m) { return (n + m - 1) / m * m; }
// element (i, j) of a lib4 matrix with panel stride sd
inline long long idx4(int sd, int i, int j) { return (long long)(i / BS) * BS * sd + i % BS + BS * j; }
inline double& P4(double* A, int sd, int i, int j) { return A[idx4(sd, i, j)]; }

inline bool hip_ok(hipError_t e, const char* what) {
    if (e == hipSuccess) return true;
    char msg[256];
    snprintf(msg, sizeof msg, "HIP error in %s: %s", what, hipGetErrorString(e));
    hk_set_error(HPMPC_MI355X_EHIP, msg);
    return false;
}

// The device copy of a host array: allocated and filled by upload(), freed with its owner, never rewritten.
template <class T>
class DevTable {
    T* d_ = nullptr;

public:
    DevTable() = default;
    DevTable(DevTable&& o) noexcept : d_(o.d_) { o.d_ = nullptr; }
    DevTable(const DevTable&) = delete;
    DevTable& operator=(const DevTable&) = delete;
    ~DevTable() {
        if (d_) (void)hipFree(d_);
    }
    bool upload(const std::vector<T>& h, const char* what) {
        return hip_ok(hipMalloc((void**)&d_, sizeof(T) * h.size()), what) &&
               hip_ok(hipMemcpy(d_, h.data(), sizeof(T) * h.size(), hipMemcpyHostToDevice), what);
    }
    const T* get() const { return d_; }
};

// The device context of the host-buffer entry points, one per host thread (g_dev, defined in hpmpc_capi.cpp): a
// stream, a device arena and its pinned staging twin, sized in bytes and only ever grown.  Nothing in the arenas
// outlives a call: every entry point sizes the context for its own carve (ensure also clears that much of the
// pinned arena), uploads the whole carve, and synchronises in down() before it returns; what persists between
// calls travels through the caller's `memory` / `double_work_memory`.
struct DevCtx {
    hipStream_t stream = nullptr;
    char* dev = nullptr;
    char* host = nullptr;
    size_t cap = 0;
    ~DevCtx() {
        if (dev) (void)hipFree(dev);
        if (host) (void)hipHostFree(host);
        if (stream) (void)hipStreamDestroy(stream);
    }
    bool ensure(size_t bytes) {
        if (!stream && !hip_ok(hipStreamCreateWithFlags(&stream, hipStreamNonBlocking), "stream create")) return false;
        if (bytes > cap) {
            if (dev) (void)hipFree(dev);
            if (host) (void)hipHostFree(host);
            dev = host = nullptr;
            cap = 0;
            if (!hip_ok(hipMalloc((void**)&dev, bytes), "device arena")) return false;
            if (!hip_ok(hipHostMalloc((void**)&host, bytes, 0), "pinned arena")) return false;
            cap = bytes;
        }
        memset(host, 0, bytes);
        return true;
    }
    bool up(size_t bytes) { return hip_ok(hipMemcpyAsync(dev, host, bytes, hipMemcpyHostToDevice, stream), "H2D"); }
    bool down(size_t bytes) {
        return hip_ok(hipMemcpyAsync(host, dev, bytes, hipMemcpyDeviceToHost, stream), "D2H") &&
               hip_ok(hipStreamSynchronize(stream), "sync");
    }
};
extern thread_local DevCtx g_dev;

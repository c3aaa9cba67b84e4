// hk_wide_host.h -- host-side helpers of the wide-stage path shared by hpmpc_capi_wide.cpp (Riccati),
// hpmpc_capi_pcond.cpp (partial condensing, through hk_pcond_plan.h) and hpmpc_capi_wide_ipm.cpp (the IPM on wide
// stages): the packed per-problem layout of a wide problem, the WideArgs fields that follow from it, the typed carve
// of the staging arena (the thread's device context, g_dev of hk_host.h), the copies between the caller's per-stage
// buffers and the packed layout, and the launch wrapper.
#pragma once
#include <algorithm>
#include <cstdlib>
#include <vector>

#include "hk_host.h"
#include "hk_wide_args.h"

namespace {

constexpr int LDS_MAX_DOUBLES = 65536 / 8;

inline int poff(int j, int nz) { return j * nz - (j * (j - 1)) / 2; }

// Lengths (doubles) of stage k's lib4 blocks BAbt_k / RSQrq_k / DCt_k and of its constraint vector
// [lb | ub | lg | ug] (d, lam, t and their kin).
inline size_t len_BAbt(const WideStage& s) { return (size_t)rup(s.nu + s.nx + 1, BS) * s.sdB; }
inline size_t len_RSQ(const WideStage& s) { return (size_t)rup(s.nu + s.nx + 1, BS) * s.sdR; }
inline size_t len_DCt(const WideStage& s) { return (size_t)rup(s.nu + s.nx, BS) * s.sdG; }
inline int len_cvec(const WideStage& s) { return 2 * s.pnb + 2 * rup(s.ng, BS); }

// One problem's packed layout on the wide path (offsets in doubles; idxb in ints).
struct WLayout {
    int N = 0;
    std::vector<WideStage> st;
    long long nB = 0, nR = 0, nL = 0, nU = 0, nP = 0, nD = 0, nI = 0, nG = 0;
    int lds = 0, offW = 0, offX = 0, offV = 0, ldW = 0, ldX = 0, offST = 0;
    bool any_ng = false;
    bool fits = true;  // hk_wide_sv limits: nu+nx+1 <= 128 (two rows per lane), nx <= 64 (MFMA tiles per wave)
};

WLayout make_layout(int N, const int* nx, const int* nu, const int* nb, const int* ng) {
    WLayout L;
    L.N = N;
    L.st.resize(N + 1);
    int Mmax = 1, nzM = 1, nxM = 1;
    for (int k = 0; k <= N; k++) {
        WideStage& s = L.st[k];
        memset(&s, 0, sizeof s);
        s.nu = k < N ? nu[k] : 0;
        s.nx = nx[k];
        s.nx1 = k < N ? nx[k + 1] : 0;
        s.nu1 = k + 1 < N ? nu[k + 1] : 0;
        const int nux = s.nu + s.nx;
        s.sdB = rup(s.nx1, NCL);
        s.sdR = rup(nux, NCL);
        s.nb = nb[k];
        s.pnb = rup(nb[k], BS);
        s.ng = ng[k];
        s.sdG = rup(ng[k], NCL);
        s.oB = (int)L.nB;
        if (k < N) L.nB += len_BAbt(s);
        s.oR = (int)L.nR;
        L.nR += len_RSQ(s);
        s.oL = (int)L.nL;
        L.nL += poff(nux, nux + 1) + nux;
        L.nL = (L.nL + 7) / 8 * 8;
        s.oU = (int)L.nU;
        L.nU += rup(nux + 1, 8);
        s.oP = (int)L.nP;
        L.nP += rup(s.nx1 + 1, 8);
        s.oG = (int)L.nG;
        L.nG += len_DCt(s);
        s.oD = (int)L.nD;
        L.nD += len_cvec(s);
        s.oI = (int)L.nI;
        L.nI += nb[k];
        if (ng[k] > 0) L.any_ng = true;
        Mmax = std::max(Mmax, poff(nux, nux + 1));
        nzM = std::max(nzM, nux + 1);
        nxM = std::max(nxM, std::max(s.nx1, s.nx));  // X also receives stage k's own Lxx
    }
    L.fits = nzM <= 128 && nxM <= 64;
    L.ldW = nzM;
    L.ldX = nxM + 1;
    L.offW = Mmax + nzM;  // the forward stages L_k with its 1/diag tail into M
    L.offX = L.offW + L.ldW * nxM;
    L.offV = L.offX + L.ldX * nxM;
    L.offST = rup(L.offV + nzM, 2);  // the stage table (WideStage records) in LDS
    L.lds = L.offST + (N + 1) * (int)(sizeof(WideStage) / sizeof(double));
    if (L.nD == 0) L.nD = 1;
    if (L.nI == 0) L.nI = 1;
    if (L.nB == 0) L.nB = 1;
    if (L.nG == 0) L.nG = 1;
    return L;
}

// The sizes, per-problem strides and LDS carve of a zeroed WideArgs.
inline void wide_args(const WLayout& L, int nprob, int p0, WideArgs& a) {
    a.N = L.N;
    a.nprob = nprob;
    a.p0 = p0;
    a.sB = L.nB;
    a.sR = L.nR;
    a.sW = L.nL;
    a.sU = L.nU;
    a.sP = L.nP;
    a.sC = L.nD;
    a.sG = L.nG;
    a.offW = L.offW;
    a.offX = L.offX;
    a.offV = L.offV;
    a.offST = L.offST;
    a.ldW = L.ldW;
    a.ldX = L.ldX;
}

// The staging arena of one call: n elements of T at the same offset of g_dev's pinned arena (host(), staged and
// read back there) and of its device twin (dev(), what the argument block points to).  Every slot starts on a
// 256-byte boundary; the pointers are valid once g_dev.ensure(Carve::o) has sized the arenas.
template <class T>
struct Slot {
    size_t off = 0;
    T* host() const { return reinterpret_cast<T*>(g_dev.host + off); }
    T* dev() const { return reinterpret_cast<T*>(g_dev.dev + off); }
    void put(const std::vector<T>& v) const {
        if (!v.empty()) memcpy(host(), v.data(), sizeof(T) * v.size());
    }
};
struct Carve {
    size_t o = 0;
    template <class T>
    Slot<T> take(size_t n) {
        Slot<T> s{o};
        o += (n * sizeof(T) + 255) / 256 * 256;
        return s;
    }
};

// The caller's per-stage buffers (lib4 blocks, possibly aliased stage pointers) into the packed layout ...
inline void BAbt_in(const WLayout& L, double* H, double* const* p) {
    for (int k = 0; k < L.N; k++) memcpy(H + L.st[k].oB, p[k], len_BAbt(L.st[k]) * sizeof(double));
}
inline void RSQ_in(const WLayout& L, double* H, double* const* p) {
    for (int k = 0; k <= L.N; k++) memcpy(H + L.st[k].oR, p[k], len_RSQ(L.st[k]) * sizeof(double));
}
inline void DCt_in(const WLayout& L, double* H, double* const* p) {  // stages with ng > 0
    for (int k = 0; k <= L.N; k++)
        if (L.st[k].ng > 0) memcpy(H + L.st[k].oG, p[k], len_DCt(L.st[k]) * sizeof(double));
}
inline void idxb_in(const WLayout& L, int* H, int* const* idxb) {  // stages with nb > 0
    for (int k = 0; k <= L.N; k++)
        if (L.st[k].nb > 0) memcpy(H + L.st[k].oI, idxb[k], L.st[k].nb * sizeof(int));
}
// ... and the per-stage vectors in and out: ux_k (nu + nx), pi_k (nx_{k+1}, k < N), constraint vectors (stages with
// nb + ng > 0; a null v stages nothing)
inline void uvec_in(const WLayout& L, double* H, double* const* v) {
    for (int k = 0; k <= L.N; k++) memcpy(H + L.st[k].oU, v[k], (L.st[k].nu + L.st[k].nx) * sizeof(double));
}
inline void uvec_out(const WLayout& L, const double* H, double* const* v) {
    for (int k = 0; k <= L.N; k++) memcpy(v[k], H + L.st[k].oU, (L.st[k].nu + L.st[k].nx) * sizeof(double));
}
inline void pvec_in(const WLayout& L, double* H, double* const* v) {
    for (int k = 0; k < L.N; k++) memcpy(H + L.st[k].oP, v[k], L.st[k].nx1 * sizeof(double));
}
inline void pvec_out(const WLayout& L, const double* H, double* const* v) {
    for (int k = 0; k < L.N; k++) memcpy(v[k], H + L.st[k].oP, L.st[k].nx1 * sizeof(double));
}
inline void cvec_in(const WLayout& L, double* H, double* const* v) {
    for (int k = 0; v && k <= L.N; k++)
        if (L.st[k].nb + L.st[k].ng > 0) memcpy(H + L.st[k].oD, v[k], len_cvec(L.st[k]) * sizeof(double));
}
inline void cvec_out(const WLayout& L, const double* H, double* const* v) {
    for (int k = 0; k <= L.N; k++)
        if (L.st[k].nb + L.st[k].ng > 0) memcpy(v[k], H + L.st[k].oD, len_cvec(L.st[k]) * sizeof(double));
}

bool launch(int which, const void* args, int count, int lds, hipStream_t stream, const char* name) {
    if (lds > LDS_MAX_DOUBLES) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "wide stage beyond the 64 KiB LDS tile budget");
        return false;
    }
    int e = hk_wide_launch(which, args, count, lds, stream);
    if (e) {
        char msg[128];
        snprintf(msg, sizeof msg, "%s launch failed (%d)", name, e);
        hk_set_error(HPMPC_MI355X_EHIP, msg);
        return false;
    }
    return true;
}

}  // namespace

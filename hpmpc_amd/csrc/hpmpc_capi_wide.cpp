// hpmpc_capi_wide.cpp -- host side of the wide-stage Riccati (hk_wide_sv / hk_wide_trs, hk_wide.hip):
// d_back_ric_rec_sv_tv_res / _trf_tv_res / _trs_tv_res for stages beyond the 16-wide register tile (routed here by
// hpmpc_capi_dropin.cpp).  Every computation runs on the GPU; the host only packs stage tables and copies buffers.
// Partial condensing on the same stages is hpmpc_capi_pcond.cpp.
#include "hk_wide_host.h"

extern "C" long long hk_wide_factor_bytes(int N, const int* nx, const int* nu) {
    long long s = 0;
    for (int k = 0; k <= N; k++) {
        const int nux = (k < N ? nu[k] : 0) + nx[k];
        s += poff(nux, nux + 1) + nux;
        s = (s + 7) / 8 * 8;
    }
    return s * 8;
}

namespace {
// General constraints of the drop-in Riccati calls: DCt_k and the general halves of Qx / qx ([box (pnb) |
// general (png)]) staged for the device (DCt diag(Qx_g) DCt' and DCt qx_g are added there, d_back_ric_rec.c:
// 210-231, :292-317, :620-633); the box halves stay on the host path (the reference's in-place side effects).
struct GenStage {
    Slot<double> G, Qx, qx;
};
GenStage carve_general(const WLayout& L, Carve& c) {
    GenStage g;
    if (!L.any_ng) return g;
    g.G = c.take<double>(L.nG);
    g.Qx = c.take<double>(L.nD);
    g.qx = c.take<double>(L.nD);
    return g;
}
void stage_general(const WLayout& L, const GenStage& g, double** hpDCt, double** Qx, double** qx, WideArgs& a) {
    if (!L.any_ng) return;
    DCt_in(L, g.G.host(), hpDCt);
    for (int k = 0; k <= L.N; k++) {
        const WideStage& s = L.st[k];
        for (int l = 0; l < s.ng; l++) {
            if (Qx) g.Qx.host()[s.oD + s.pnb + l] = Qx[k][s.pnb + l];
            if (qx) g.qx.host()[s.oD + s.pnb + l] = qx[k][s.pnb + l];
        }
    }
    a.DCt = g.G.dev();
    a.Qx = g.Qx.dev();
    a.qx = g.qx.dev();
}
bool fits_check(const WLayout& L) {
    if (L.lds > LDS_MAX_DOUBLES || !L.fits) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "wide stage beyond the kernel's tile limits (64 KiB LDS, "
                                                "nu+nx < 128, nx <= 64)");
        return false;
    }
    return true;
}
// one problem's arguments: the layout's fields, then the stage table (staged here) and the vectors every call has
struct RicSlots {
    Slot<WideStage> st;
    Slot<double> B, F, U, Pi;
};
void ric_args(const WLayout& L, const RicSlots& r, WideArgs& a) {
    memset(&a, 0, sizeof a);
    wide_args(L, 1, 0, a);
    r.st.put(L.st);
    a.st = r.st.dev();
    a.BAbt = r.B.dev();
    a.ws = r.F.dev();
    a.ux = r.U.dev();
    a.pi = r.Pi.dev();
}
}  // namespace

// d_back_ric_rec_sv_tv_res on wide stages (called by hpmpc_capi_dropin.cpp when the tile path does not fit).
extern "C" void hk_wide_sv_entry(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, int update_b, double** hpBAbt,
                                 double** b, int update_q, double** hpQ, double** q, double** bd, double** hpDCt,
                                 double** Qx, double** qx, double** hux, int compute_pi, double** hpi, int compute_Pb,
                                 double** hPb, double* memory) {
    hk_set_error(0, nullptr);
    WLayout L = make_layout(N, nx, nu, nb, ng);
    if (!fits_check(L)) return;
    Carve c;
    RicSlots r;
    r.st = c.take<WideStage>(N + 1);
    r.B = c.take<double>(L.nB);
    const Slot<double> R = c.take<double>(L.nR);
    r.F = c.take<double>(L.nL);
    r.U = c.take<double>(L.nU);
    r.Pi = c.take<double>(L.nP);
    const Slot<double> Pb = c.take<double>(L.nP);
    const GenStage gs = carve_general(L, c);
    if (!g_dev.ensure(c.o)) return;
    // the reference's in-place side effects, in its stage order (d_back_ric_rec.c:197-209, :249-291)
    for (int k = N; k >= 0; k--) {
        const WideStage& s = L.st[k];
        const int nux = s.nu + s.nx;
        if (update_q)
            for (int j = 0; j < nux; j++) P4(hpQ[k], s.sdR, nux, j) = q[k][j];
        for (int l = 0; l < nb[k]; l++) {
            const int ii = idxb[k][l];
            P4(hpQ[k], s.sdR, ii, ii) = bd[k][l] + Qx[k][l];
        }
        for (int l = 0; l < nb[k]; l++) P4(hpQ[k], s.sdR, nux, idxb[k][l]) += qx[k][l];
        memcpy(R.host() + s.oR, hpQ[k], len_RSQ(s) * sizeof(double));
        if (k < N) {
            if (update_b)
                for (int j = 0; j < s.nx1; j++) P4(hpBAbt[k], s.sdB, nux, j) = b[k][j];
            memcpy(r.B.host() + s.oB, hpBAbt[k], len_BAbt(s) * sizeof(double));
        }
    }
    WideArgs a;
    ric_args(L, r, a);
    stage_general(L, gs, hpDCt, Qx, qx, a);
    a.RSQ = R.dev();
    a.Pb = Pb.dev();
    a.compute_pi = compute_pi;
    a.compute_Pb = compute_Pb;
    if (!g_dev.up(c.o) || !launch(WL_SV, &a, 1, L.lds, g_dev.stream, "hk_wide_sv") || !g_dev.down(c.o)) return;
    uvec_out(L, r.U.host(), hux);
    if (compute_pi) pvec_out(L, r.Pi.host(), hpi);
    if (compute_Pb) pvec_out(L, Pb.host(), hPb);
    memcpy(memory, r.F.host(), 8 * L.nL);
}

// d_back_ric_rec_trf_tv_res on wide stages: hk_wide_sv in factor-only mode (no augmented row, no forward).
extern "C" void hk_wide_trf_entry(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                  double** hpQ, double** hpDCt, double** Qx, double** bd, double* memory) {
    hk_set_error(0, nullptr);
    WLayout L = make_layout(N, nx, nu, nb, ng);
    if (!fits_check(L)) return;
    Carve c;
    RicSlots r;
    r.st = c.take<WideStage>(N + 1);
    r.B = c.take<double>(L.nB);
    const Slot<double> R = c.take<double>(L.nR);
    r.F = c.take<double>(L.nL);
    r.U = c.take<double>(L.nU);
    r.Pi = c.take<double>(L.nP);
    const GenStage gs = carve_general(L, c);
    if (!g_dev.ensure(c.o)) return;
    for (int k = N; k >= 0; k--) {  // the reference's side effect: box diagonal = bd + Qx (d_back_ric_rec.c:468, :520)
        const WideStage& s = L.st[k];
        for (int l = 0; l < nb[k]; l++) {
            const int ii = idxb[k][l];
            P4(hpQ[k], s.sdR, ii, ii) = bd[k][l] + Qx[k][l];
        }
        memcpy(R.host() + s.oR, hpQ[k], len_RSQ(s) * sizeof(double));
    }
    BAbt_in(L, r.B.host(), hpBAbt);
    WideArgs a;
    ric_args(L, r, a);
    stage_general(L, gs, hpDCt, Qx, nullptr, a);
    a.trf = 1;
    a.RSQ = R.dev();
    a.Pb = a.pi;
    if (!g_dev.up(c.o) || !launch(WL_SV, &a, 1, L.lds, g_dev.stream, "hk_wide_sv(trf)") || !g_dev.down(c.o)) return;
    memcpy(memory, r.F.host(), 8 * L.nL);
}

// d_back_ric_rec_trs_tv_res on wide stages (hk_wide_trs) over the factor hk_wide_trf_entry left in memory.
extern "C" void hk_wide_trs_entry(int N, int* nx, int* nu, int* nb, int** idxb, int* ng, double** hpBAbt,
                                  double** hb, double** hq, double** hpDCt, double** qx, double** hux, int compute_pi,
                                  double** hpi, int compute_Pb, double** hPb, double* memory) {
    hk_set_error(0, nullptr);
    WLayout L = make_layout(N, nx, nu, nb, ng);
    if (!fits_check(L)) return;
    Carve c;
    RicSlots r;
    r.st = c.take<WideStage>(N + 1);
    r.B = c.take<double>(L.nB);
    r.F = c.take<double>(L.nL);
    r.U = c.take<double>(L.nU);
    r.Pi = c.take<double>(L.nP);
    const Slot<double> Pb = c.take<double>(L.nP), vb = c.take<double>(L.nP), vq = c.take<double>(L.nU),
                       vqx = c.take<double>(L.nD);
    const Slot<int> I = c.take<int>(L.nI);
    const Slot<double> G = c.take<double>(L.nG);
    if (!g_dev.ensure(c.o)) return;
    memcpy(r.F.host(), memory, 8 * L.nL);
    BAbt_in(L, r.B.host(), hpBAbt);
    pvec_in(L, vb.host(), hb);
    uvec_in(L, vq.host(), hq);
    if (!compute_Pb) pvec_in(L, Pb.host(), hPb);
    idxb_in(L, I.host(), idxb);
    DCt_in(L, G.host(), hpDCt);  // DCt qx_g on the device (general half of qx at pnb)
    for (int k = 0; k <= N; k++) {
        const WideStage& s = L.st[k];
        if (s.nb > 0) memcpy(vqx.host() + s.oD, qx[k], s.nb * sizeof(double));
        if (s.ng > 0) memcpy(vqx.host() + s.oD + s.pnb, qx[k] + s.pnb, s.ng * sizeof(double));
    }
    WideArgs a;
    ric_args(L, r, a);
    a.Pb = Pb.dev();
    a.hb = vb.dev();
    a.hq = vq.dev();
    a.qx = vqx.dev();
    a.idxb = I.dev();
    if (L.any_ng) a.DCt = G.dev();
    a.compute_pi = compute_pi;
    a.compute_Pb = compute_Pb;
    if (!g_dev.up(c.o) || !launch(WL_TRS, &a, 1, L.lds, g_dev.stream, "hk_wide_trs") || !g_dev.down(c.o)) return;
    uvec_out(L, r.U.host(), hux);
    if (compute_pi) pvec_out(L, r.Pi.host(), hpi);
    if (compute_Pb) pvec_out(L, Pb.host(), hPb);
}

// hk_pcond_plan.h -- host-only bookkeeping of partial condensing (hpmpc_capi_pcond.cpp): the block split and the
// condensed sizes (d_part_cond.c:694-738), the plan of one problem shape with hk_pcond's and hk_pexpand's LDS carves
// and the limits they are refused at, and the PcArgs / PxArgs fields that follow from a plan.  No device work.
#pragma once
#include "hk_wide_host.h"

namespace {

int block_len(int N, int N2, int ii) {
    const int N1 = N / N2, R1 = N - N2 * N1, M1 = R1 > 0 ? N1 + 1 : N1;
    return ii < R1 ? M1 : N1;
}

struct PcPlan {
    int N = 0, N2 = 0;
    WLayout orig, cond;
    std::vector<int> nx2, nu2, nb2, ng2;
    std::vector<int> idxb2;  // condensed box indices packed per stage (cond.st[ii].oI), as hk_pcond writes them
    std::vector<PcBlock> blk;
    std::vector<int> idxb;  // original idxb packed per stage (orig.st[k].oI)
    long long nG = 0;       // Gamma scratch (doubles per problem)
    long long nG2 = 0;      // condensed DCt2 (doubles per problem)
    long long ref_d = 0;    // the reference's memory carve: doubles before the idxb2 ints
    int pc_lds = 0, ldP = 0, ldX = 0, ldW = 0, ldB = 0, offP = 0, offX = 0, offW = 0, offB = 0, offGA = 0, offGB = 0;
    int px_lds = 0, ldT = 0, xoB = 0, xoR = 0, xoV = 0, xoW = 0, xoQ = 0;
    int pc_gm = 4;  // hk_pcond's gemm tiles per wave (4 or 8)
    int offST = 0;  // hk_pcond's LDS stage table
    int offU = 0;   // hk_pcond's P-form u columns
    int offGT = 0;  // hk_pcond's P-form certificate bounds
    bool pform_ok = true;
    bool pc_dm_ok = true;  // hk_pcond's deferred cross terms fit the Gamma scratch and leave DCtd's bookkeeping alone
};

void problem_size(int N, const int* nx, const int* nu, const int* nb, const int* const* hidxb, const int* ng, int N2,
                  int* nx2, int* nu2, int* nb2, int* ng2) {
    int N_tmp = 0;
    for (int ii = 0; ii < N2; ii++) {
        const int T1 = block_len(N, N2, ii);
        nx2[ii] = nx[N_tmp];
        nu2[ii] = nu[N_tmp];
        nb2[ii] = nb[N_tmp];
        ng2[ii] = ng[N_tmp];
        for (int jj = 1; jj < T1; jj++) {
            const int s = N_tmp + jj;
            int nbb = 0, nbg = 0;
            for (int kk = 0; kk < nb[s]; kk++) (hidxb[s][kk] < nu[s] ? nbb : nbg)++;
            nu2[ii] += nu[s];
            nb2[ii] += nbb;
            ng2[ii] += ng[s] + nbg;
        }
        N_tmp += T1;
    }
    nx2[N2] = nx[N];
    nu2[N2] = nu[N];
    nb2[N2] = nb[N];
    ng2[N2] = ng[N];
}

bool pc_plan(PcPlan& P, int N, const int* nx, const int* nu_in, const int* nb, const int* const* idxb, const int* ng,
             int N2) {
    if (N2 < 1 || N2 > N) {  // N2 == N: blocks of one stage (d_part_cond itself aliases instead, :936)
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "partial condensing needs 1 <= N2 <= N (:962-967)");
        return false;
    }
    for (int k = 0; k < N; k++)
        if (ng[k] > 0) {  // d_part_cond.c:971-976: only ng[N] > 0 is supported by the reference
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "partial condensing with ng > 0 before the last stage");
            return false;
        }
    std::vector<int> nu(nu_in, nu_in + N + 1);
    nu[N] = 0;
    P.N = N;
    P.N2 = N2;
    P.orig = make_layout(N, nx, nu.data(), nb, ng);
    P.idxb.assign(P.orig.nI, 0);
    for (int k = 0; k <= N; k++)
        for (int l = 0; l < nb[k]; l++) P.idxb[P.orig.st[k].oI + l] = idxb[k][l];
    P.nx2.resize(N2 + 1);
    P.nu2.resize(N2 + 1);
    P.nb2.resize(N2 + 1);
    P.ng2.resize(N2 + 1);
    problem_size(N, nx, nu.data(), nb, idxb, ng, N2, P.nx2.data(), P.nu2.data(), P.nb2.data(), P.ng2.data());
    P.cond = make_layout(N2, P.nx2.data(), P.nu2.data(), P.nb2.data(), P.ng2.data());
    P.blk.resize(N2);
    int N_tmp = 0, nzM = 1, nxM = 1;
    long long oG2 = 0, ref_d = 0;
    for (int ii = 0; ii < N2; ii++) {
        PcBlock& b = P.blk[ii];
        memset(&b, 0, sizeof b);
        b.s0 = N_tmp;
        b.T = block_len(N, N2, ii);
        b.nx0 = nx[N_tmp];
        b.nut = 0;
        b.oG = (int)P.nG;
        int rows = b.nx0 + 1;
        long long sneed = 0;  // hk_pcond's deferred cross terms: (nx_s + 1) x nu_s per stage s >= 1 of the block
        for (int j = 0; j < b.T; j++) {
            const int s = N_tmp + j;
            b.nut += nu[s];
            rows += nu[s];
            P.nG += (long long)rows * nx[s + 1];
            if (j > 0) sneed += (long long)(nx[s] + 1) * nu[s];
            nzM = std::max(nzM, nu[s] + nx[s] + 1);
            nxM = std::max(nxM, nx[s + 1]);
        }
        if (sneed > P.nG - b.oG) P.pc_dm_ok = false;  // the block's Gamma scratch holds them (it always does at nu <= nx)
        b.oB2 = P.cond.st[ii].oB;
        b.oR2 = P.cond.st[ii].oR;
        b.oD2 = P.cond.st[ii].oD;
        b.oI2 = P.cond.st[ii].oI;
        b.oG2 = (int)oG2;
        oG2 += (long long)rup(P.nu2[ii] + P.nx2[ii], BS) * rup(P.ng2[ii], NCL);
        b.nx2n = P.nx2[ii + 1];
        b.nb2 = P.nb2[ii];
        b.ng2 = P.ng2[ii];
        N_tmp += b.T;
        // the reference's carve of `memory` (d_part_cond.c:1013-1041), doubles part
        const int pnz2 = rup(P.nu2[ii] + P.nx2[ii] + 1, BS);
        ref_d += (long long)pnz2 * rup(P.nx2[ii + 1], NCL) + (long long)pnz2 * rup(P.nu2[ii] + P.nx2[ii], NCL) +
                 (long long)rup(P.nu2[ii] + P.nx2[ii], BS) * rup(P.ng2[ii], NCL) + 2 * rup(P.nb2[ii], BS) +
                 2 * rup(P.ng2[ii], BS);
    }
    P.nG2 = oG2 > 0 ? oG2 : 1;
    P.ref_d = ref_d;
    // condensed box indices (d_cond_DCtd, d_part_cond.c:579-688): input boxes of the block's later stages keep
    // their position in [u_{T-1}; ..; u_0; x_0], stage 0's boxes stay boxes, inner state boxes become general
    P.idxb2.assign(P.cond.nI, 0);
    for (int ii = 0; ii < N2; ii++) {
        const PcBlock& b = P.blk[ii];
        int* i2 = P.idxb2.data() + P.cond.st[ii].oI;
        int ib = 0, nu_tmp = 0;
        for (int sI = b.T - 1; sI >= 1; sI--) {
            const int s = b.s0 + sI;
            nu_tmp += nu[s];
            for (int jj = 0; jj < nb[s]; jj++)
                if (idxb[s][jj] < nu[s]) i2[ib++] = nu_tmp - nu[s] + idxb[s][jj];
        }
        nu_tmp += nu[b.s0];
        for (int jj = 0; jj < nb[b.s0]; jj++) i2[ib++] = nu_tmp - nu[b.s0] + idxb[b.s0][jj];
    }
    for (int l = 0; l < nb[N]; l++) P.idxb2[P.cond.st[N2].oI + l] = idxb[N][l];
    // Gamma tiles: the largest (rows x nx_{j+1}) of any block, also used as the RSQrq_{s-1} tile
    long long gmax = (long long)nzM * nzM;
    int tmax = 0;  // output tiles of hk_pcond's largest gemm: Gamma_{j-1} A_j, and W / W W' of d_cond_RSQrq
    auto tiles = [](int m, int n) { return ((m + 15) / 16) * ((n + 15) / 16); };
    {
        int Nt = 0;
        for (int ii = 0; ii < N2; ii++) {
            int rows = nx[Nt] + 1;
            for (int j = 0; j < P.blk[ii].T; j++) {
                const int s = Nt + j;
                if (j > 0) tmax = std::max(tmax, tiles(rows, nx[s + 1]));  // rows = rows(j - 1)
                rows += nu[s];
                gmax = std::max(gmax, (long long)rows * nx[s + 1]);
                if (j > 0) {  // d_cond_RSQrq at stage s: W (nz_{s-1} x nx_s), W W' (nz_{s-1} x nux_{s-1})
                    const int nzp = nu[s - 1] + nx[s - 1] + 1;
                    tmax = std::max(tmax, std::max(tiles(nzp, nx[s]), tiles(nzp, nzp - 1)));
                }
            }
            Nt += P.blk[ii].T;
        }
    }
    if (tmax > 32) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "condensing block beyond hk_pcond's gemm tiles (32 16x16 tiles)");
        return false;
    }
    P.pc_gm = tmax <= 16 ? 4 : 8;
    // hk_pcond's LDS carve (doubles, every tile 32-byte aligned for the 16-byte LDS DMA), in this order:
    //   offP   pL as a lib4 RSQrq block (rup(nz, 4) x sdR)
    //   offX   Lx dense, or the P form's T = X^ [BAbt | e]' ((nx+1) x nz)
    //   offB   the BAbt tile, dense (d_cond_BAbt) or as a lib4 block (d_cond_RSQrq); W is formed in place (offW)
    //   offGA  Gamma_{j-1}, also the RSQrq_{s-1} tile and the P form's per-row scratch
    //   offST  the block's stage records (WideStage, T of them)
    //   offU   the P form's u columns of pL_s; offGT its certificate bounds
    // Which phase may touch what: d_cond_DCtd keeps its integer bookkeeping (cU, cX, iob, iog, ntmp, igb: T ints each;
    // gd, gj: ng2 ints each, bk = 6 T + 2 ng2 ints) at sm[0], over the tiles, and every phase reads the stage records,
    // so a block with bk > 2 offST ints is refused.  In the reference's order DCtd runs last and the tiles are free.
    // With the cross terms deferred (dm), babt_phase runs after it and writes offB.., offGA.. and offU.. while dm_stage
    // still reads the bookkeeping, so dm needs bk <= 2 offB ints: the plan takes the reference's order otherwise.
    int nuxM = 1;
    for (int k = 0; k < N; k++) nuxM = std::max(nuxM, nu[k] + nx[k]);
    P.ldP = P.ldW = P.ldB = nzM;
    P.ldX = nxM + 1;
    P.offP = 0;
    P.offX = rup(std::max(P.ldP * nzM, rup(nzM, BS) * rup(nuxM, NCL)), 4);
    P.offB = P.offX + rup(P.ldX * nzM, 4);
    P.offW = P.offB;
    P.offGA = P.offB + rup(std::max(P.ldB * nxM, rup(nzM, BS) * rup(nxM, NCL)), 4);
    P.offGB = 0;
    int Tmax = 1;
    for (int ii = 0; ii < N2; ii++) Tmax = std::max(Tmax, P.blk[ii].T);
    P.offST = P.offGA + rup((int)gmax, 4);
    int nuM = 1;
    for (int k = 0; k < N; k++) nuM = std::max(nuM, nu[k]);
    P.offU = P.offST + rup(Tmax * (int)(sizeof(WideStage) / sizeof(double)), 2);
    P.offGT = P.offU + P.ldX * nuM;
    P.pc_lds = P.offGT + Tmax;
    // the P form's per-row scratch (one row value per stage and state) lives in the Gamma tile before d_cond_RSQrq
    P.pform_ok = (long long)(Tmax - 1) * nxM <= gmax;
    if (gmax > 12 * 256 || nxM > 63) {  // hk_pcond: PC_GCH Gamma outputs per lane; the state Cholesky in one wave
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "condensing block beyond the kernel's tile limits "
                                                "(Gamma rows x nx <= 3072, nx <= 63)");
        return false;
    }
    // expansion tiles: BAbt (nzM x nxM), RSQrq (nzM x nzM), ux_j, box terms, pi_j
    P.ldT = nzM;
    P.xoB = 0;
    P.xoR = P.xoB + nzM * nxM;
    P.xoV = P.xoR + nzM * nzM;
    P.xoW = P.xoV + nzM;
    P.xoQ = P.xoW + nzM;
    P.px_lds = P.xoQ + std::max(nzM, nxM);
    for (int ii = 0; ii < N2; ii++) {  // the two bounds on d_cond_DCtd's bookkeeping, read off the carve above
        const long long bk = 6LL * P.blk[ii].T + 2LL * P.ng2[ii];
        if (bk > 2LL * P.offST) {
            hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "condensing block with more state boxes than the LDS tiles hold");
            return false;
        }
        if (bk > 2LL * P.offB) P.pc_dm_ok = false;
    }
    if (P.pc_lds > LDS_MAX_DOUBLES || P.px_lds > LDS_MAX_DOUBLES) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "condensing stage tiles beyond the 64 KiB LDS budget");
        return false;
    }
    return true;
}

void fill_pc_args(const PcPlan& P, PcArgs& a) {
    memset(&a, 0, sizeof a);
    a.N = P.N;
    a.N2 = P.N2;
    a.sB = P.orig.nB;
    a.sR = P.orig.nR;
    a.sD = P.orig.nD;
    a.sG = P.nG;
    a.sB2 = P.cond.nB;
    a.sR2 = P.cond.nR;
    a.sG2 = P.nG2;
    a.sD2 = P.cond.nD;
    a.oR2N = P.cond.st[P.N2].oR;
    a.oD2N = P.cond.st[P.N2].oD;
    a.nDN = len_cvec(P.orig.st[P.N]);
    a.sdRN = P.orig.st[P.N].sdR;
    a.nzN = P.orig.st[P.N].nu + P.orig.st[P.N].nx + 1;
    a.offP = P.offP;
    a.offX = P.offX;
    a.offW = P.offW;
    a.offB = P.offB;
    a.ldP = P.ldP;
    a.ldX = P.ldX;
    a.ldW = P.ldW;
    a.ldB = P.ldB;
    a.offGA = P.offGA;
    a.offGB = P.offGB;
    a.ph = PC_ALL;
    a.gm = P.pc_gm;
    a.offST = P.offST;
    a.offU = P.offU;
    // HPMPC_MI355X_PCOND_PFORM=0: every stage takes the Cholesky route (read per call: tests compare the two routes)
    const char* pf = getenv("HPMPC_MI355X_PCOND_PFORM");
    a.pform = P.pform_ok && (pf ? atoi(pf) : 1);
    a.offGT = P.offGT;
    // d_cond_RSQrq before d_cond_BAbt with the cross terms deferred (no Gamma through HBM) unless
    // HPMPC_MI355X_PCOND_DM=0 (read per call: tests compare the two orders bitwise)
    const char* dmv = getenv("HPMPC_MI355X_PCOND_DM");
    a.dm = P.pc_dm_ok && (dmv ? atoi(dmv) : 1);
}

void fill_px_args(const PcPlan& P, PxArgs& a) {
    memset(&a, 0, sizeof a);
    a.N = P.N;
    a.N2 = P.N2;
    a.sB = P.orig.nB;
    a.sR = P.orig.nR;
    a.sU = P.orig.nU;
    a.sP = P.orig.nP;
    a.sC = P.orig.nD;
    a.sU2 = P.cond.nU;
    a.sP2 = P.cond.nP;
    a.sC2 = P.cond.nD;
    a.offB = P.xoB;
    a.offR = P.xoR;
    a.offV = P.xoV;
    a.offW = P.xoW;
    a.offQ = P.xoQ;
    a.ldT = P.ldT;
}

}  // namespace

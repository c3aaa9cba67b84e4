// hpmpc_capi_pcond.cpp -- host side of partial condensing on the wide-stage path (hk_pcond / hk_pexpand, hk_wide.hip):
//   * the §8f #1 row: d_part_cond_compute_problem_size / _work_space_size_bytes / _memory_space_size_bytes /
//     d_part_cond / d_part_expand_work_space_size_bytes / d_part_expand_solution (lqcp_solvers/d_part_cond.c:694-1308)
//     and the building blocks d_cond_BAbt / d_cond_RSQrq / d_cond_DCtd (:214-688), with the reference prototypes, on
//     host lib4 buffers;
//   * the batched device API of the same pipeline (hpmpc_mi355x_pcond_*), data resident in HBM.
// Every computation runs on the GPU; the host only packs stage tables and copies buffers (hk_pcond_plan.h holds the
// bookkeeping shared by the single-problem and the batched entry points).
#include "hk_pcond_plan.h"

// d_part_cond.c:694-738 -- integer bookkeeping (no device work)
extern "C" void d_part_cond_compute_problem_size(int N, int* nx, int* nu, int* nb, int** hidxb, int* ng, int N2,
                                                 int* nx2, int* nu2, int* nb2, int* ng2) {
    problem_size(N, nx, nu, nb, hidxb, ng, N2, nx2, nu2, nb2, ng2);
}

// every temporary of the condensing lives on the device
extern "C" int d_part_cond_work_space_size_bytes(int N, int* nx, int* nu, int* nb, int** hidxb, int* ng, int N2,
                                                 int* nx2, int* nu2, int* nb2, int* ng2) {
    return 64;
}

// d_part_cond.c:868-924: the condensed data are written into `memory` with the reference's carve
extern "C" int d_part_cond_memory_space_size_bytes(int N, int* nx, int* nu, int* nb, int** hidxb, int* ng, int N2,
                                                   int* nx2, int* nu2, int* nb2, int* ng2) {
    if (N2 == N) return 0;
    long long d_size = 0, i_size = 0;
    for (int ii = 0; ii < N2; ii++) {
        const int pnz2 = rup(nu2[ii] + nx2[ii] + 1, BS), pnux2 = rup(nu2[ii] + nx2[ii], BS);
        d_size += (long long)pnz2 * rup(nx2[ii + 1], NCL) + (long long)pnz2 * rup(nu2[ii] + nx2[ii], NCL) +
                  (long long)pnux2 * rup(ng2[ii], NCL) + 2 * rup(nb2[ii], BS) + 2 * rup(ng2[ii], BS);
        i_size += nb2[ii];
    }
    return (int)((d_size * 8 + i_size * 4 + 63) / 64 * 64);
}

namespace {
// the arena slots and arguments every condensing call shares: the original stages, the blocks, idxb, BAbt / RSQrq / d
// and the Gamma scratch
struct PcSlots {
    Slot<WideStage> st;
    Slot<PcBlock> blk;
    Slot<int> idx;
    Slot<double> B, R, D, G;
};
PcSlots pc_slots(const PcPlan& P, Carve& c, int pad) {
    PcSlots s;
    s.st = c.take<WideStage>(P.N + 1);
    s.blk = c.take<PcBlock>(P.N2);
    s.idx = c.take<int>(P.orig.nI + pad);
    s.B = c.take<double>(P.orig.nB);
    s.R = c.take<double>(P.orig.nR);
    s.D = c.take<double>(P.orig.nD + pad);
    s.G = c.take<double>(P.nG);
    return s;
}
void pc_stage(const PcPlan& P, const PcSlots& s, const std::vector<PcBlock>& blk, PcArgs& a) {
    s.st.put(P.orig.st);
    s.blk.put(blk);
    s.idx.put(P.idxb);
    fill_pc_args(P, a);
    a.nprob = 1;
    a.st = s.st.dev();
    a.blk = s.blk.dev();
    a.idxb = s.idx.dev();
    a.BAbt = s.B.dev();
    a.RSQ = s.R.dev();
    a.d = s.D.dev();
    a.G = s.G.dev();
}
}  // namespace

// d_part_cond.c:926-1062
extern "C" void d_part_cond(int N, int* nx, int* nu, int* nb, int** hidxb, int* ng, double** hpBAbt, double** hpRSQrq,
                            double** hpDCt, double** hd, int N2, int* nx2, int* nu2, int* nb2, int** hidxb2, int* ng2,
                            double** hpBAbt2, double** hpRSQrq2, double** hpDCt2, double** hd2, void* memory,
                            void* work) {
    (void)work;
    hk_set_error(0, nullptr);
    if (N2 == N) {  // :936-960: the condensed problem aliases the original
        for (int ii = 0; ii <= N; ii++) {
            nx2[ii] = nx[ii];
            nu2[ii] = nu[ii];
            nb2[ii] = nb[ii];
            hidxb2[ii] = hidxb[ii];
            ng2[ii] = ng[ii];
            if (ii < N) hpBAbt2[ii] = hpBAbt[ii];
            hpRSQrq2[ii] = hpRSQrq[ii];
            hpDCt2[ii] = hpDCt[ii];
            hd2[ii] = hd[ii];
        }
        return;
    }
    PcPlan P;
    if (!pc_plan(P, N, nx, nu, nb, hidxb, ng, N2)) return;
    const WLayout &O = P.orig, &C = P.cond;
    // the condensed outputs go into one buffer with the reference's carve (BAbt2 | RSQrq2 | DCt2 | d2 | idxb2,
    // d_part_cond.c:1013-1041), downloaded into `memory` as is; the kernel's copy of the terminal RSQrq
    // lands past it (the reference aliases hpRSQrq[N] there instead)
    const long long term_off = P.ref_d + (4 * C.nI + 7) / 8 + 8;
    Carve c;
    const PcSlots s = pc_slots(P, c, 0);
    const Slot<double> mem = c.take<double>(term_off + len_RSQ(O.st[N]));
    if (!g_dev.ensure(c.o)) return;
    // so the block offsets are absolute within that buffer
    std::vector<PcBlock> blk = P.blk;
    long long o = 0;
    int oi = 0;
    for (int ii = 0; ii < N2; ii++) {
        blk[ii].oB2 = (int)o;
        o += (long long)rup(P.nu2[ii] + P.nx2[ii] + 1, BS) * rup(P.nx2[ii + 1], NCL);
    }
    for (int ii = 0; ii < N2; ii++) {
        blk[ii].oR2 = (int)o;
        o += (long long)rup(P.nu2[ii] + P.nx2[ii] + 1, BS) * rup(P.nu2[ii] + P.nx2[ii], NCL);
    }
    for (int ii = 0; ii < N2; ii++) {
        blk[ii].oG2 = (int)o;
        o += (long long)rup(P.nu2[ii] + P.nx2[ii], BS) * rup(P.ng2[ii], NCL);
    }
    for (int ii = 0; ii < N2; ii++) {
        blk[ii].oD2 = (int)o;
        o += 2 * rup(P.nb2[ii], BS) + 2 * rup(P.ng2[ii], BS);
        blk[ii].oI2 = oi;
        oi += P.nb2[ii];
    }
    BAbt_in(O, s.B.host(), hpBAbt);
    RSQ_in(O, s.R.host(), hpRSQrq);
    cvec_in(O, s.D.host(), hd);
    PcArgs a;
    pc_stage(P, s, blk, a);
    a.BAbt2 = a.RSQ2 = a.DCt2 = a.d2 = mem.dev();
    a.idxb2 = reinterpret_cast<int*>(mem.dev() + P.ref_d);  // the reference's carve: the ints follow the doubles
    a.oR2N = (int)term_off;
    a.nDN = 0;  // the reference aliases hd2[N2] = hd[N] (d_part_cond.c), nothing to copy into the carve
    if (!g_dev.up(c.o) || !launch(WL_PCOND, &a, 1, P.pc_lds, g_dev.stream, "hk_pcond") || !g_dev.down(c.o)) return;
    for (int ii = 0; ii <= N2; ii++) {
        nx2[ii] = P.nx2[ii];
        nu2[ii] = P.nu2[ii];
        nb2[ii] = P.nb2[ii];
        ng2[ii] = P.ng2[ii];
    }
    memcpy(memory, mem.host(), 8 * P.ref_d + 4 * (C.nI > 0 ? oi : 0));
    double* m = static_cast<double*>(memory);
    int* mi = reinterpret_cast<int*>(m + P.ref_d);
    for (int ii = 0; ii < N2; ii++) {
        hpBAbt2[ii] = m + blk[ii].oB2;
        hpRSQrq2[ii] = m + blk[ii].oR2;
        hpDCt2[ii] = m + blk[ii].oG2;
        hd2[ii] = m + blk[ii].oD2;
        hidxb2[ii] = mi + blk[ii].oI2;
    }
    hpRSQrq2[N2] = hpRSQrq[N];
    hpDCt2[N2] = hpDCt[N];
    hd2[N2] = hd[N];
    hidxb2[N2] = hidxb[N];
}

// ------------------------------------------------------------------------------------------------
// The building blocks of one condensing block (d_cond_BAbt / d_cond_RSQrq / d_cond_DCtd, d_part_cond.c:214-688):
// the block is a horizon-N problem condensed with N2 = 1 by hk_pcond restricted to one phase (PC_PART).  Gammas
// move between the caller's lib4 matrices and the kernel's dense column-major scratch on the host; the outputs
// the reference writes only in part are uploaded first, so what it leaves alone comes back unchanged.
// ------------------------------------------------------------------------------------------------
namespace {
void cond_part(int ph, int N, const int* nx, const int* nu, const int* nb, int* const* hidxb, double* const* hpBAbt,
               double* const* hpRSQrq, double* const* hd, double** hpGamma, double* pBAbt2, double* pRSQrq2,
               double* pDCt2, double* d2, int* idxb2) {
    hk_set_error(0, nullptr);
    if (N < 1) return;  // the reference returns early (d_part_cond.c:315, :583)
    std::vector<int> nxv(nx, nx + N + 1), nuv(nu, nu + N), nbv(N + 1, 0), ngv(N + 1, 0);
    nuv.push_back(0);
    std::vector<const int*> idx(N + 1, nullptr);
    if (ph == PC_DCTD)
        for (int k = 0; k < N; k++) {
            nbv[k] = nb[k];
            idx[k] = hidxb[k];
        }
    PcPlan P;
    if (!pc_plan(P, N, nxv.data(), nuv.data(), nbv.data(), idx.data(), ngv.data(), 1)) return;
    const WLayout& O = P.orig;
    const PcBlock& b0 = P.blk[0];
    const int nv = b0.nut + b0.nx0, nbb = b0.nb2, nbg = b0.ng2;
    const int pnbb = rup(nbb, BS), pnbg = rup(nbg, BS), cnbg = rup(nbg, NCL), cnux2 = rup(nv, NCL);
    // Gamma_j: rows r_j, dense at go[j] in the scratch
    std::vector<int> rj(N);
    std::vector<long long> go(N + 1, 0);
    for (int j = 0, acc = b0.nx0 + 1; j < N; j++) {
        acc += nuv[j];
        rj[j] = acc;
        go[j + 1] = go[j] + (long long)acc * nxv[j + 1];
    }
    // extents the reference touches in the partly-written outputs (last element + 1)
    long long nR2 = idx4(cnux2, nv, nv - 1) + 1, nG2 = 0,
              nD2 = nbg > 0 ? 2 * pnbb + pnbg + nbg : (nbb > 0 ? pnbb + nbb : 0);
    if (ph == PC_DCTD) {  // d_part_cond.c:637-668: the column of general constraint ig spans rows nu_tmp .. +idx_gammab
        int ig = 0, nu_tmp = 0, idx_gammab = b0.nx0;
        for (int j = 0; j < N - 1; j++) idx_gammab += nuv[j];
        for (int s = N - 1; s >= 1; s--) {
            nu_tmp += nuv[s];
            for (int jj = 0; jj < nb[s]; jj++)
                if (hidxb[s][jj] >= nuv[s]) {
                    if (idx_gammab > 0) nG2 = std::max(nG2, idx4(cnbg, nu_tmp + idx_gammab - 1, ig) + 1);
                    ig++;
                }
            idx_gammab -= nuv[s - 1];
        }
    }
    Carve c;
    const PcSlots s = pc_slots(P, c, 1);
    const Slot<double> B2 = c.take<double>((size_t)rup(nv + 1, BS) * rup(nxv[N], NCL)), R2 = c.take<double>(nR2),
                       G2 = c.take<double>(nG2 + 1), D2 = c.take<double>(nD2 + 1);
    const Slot<int> I2 = c.take<int>(nbb + 1);
    if (!g_dev.ensure(c.o)) return;
    PcBlock blk = b0;
    blk.oB2 = blk.oR2 = blk.oG2 = blk.oD2 = blk.oI2 = 0;
    for (int k = 0; k < N; k++) {  // the block's stages only, and of each input what the phase reads
        const WideStage& w = O.st[k];
        if (ph != PC_DCTD) memcpy(s.B.host() + w.oB, hpBAbt[k], len_BAbt(w) * sizeof(double));
        if (ph == PC_RSQ) memcpy(s.R.host() + w.oR, hpRSQrq[k], len_RSQ(w) * sizeof(double));
        if (ph == PC_DCTD && nb[k] > 0) memcpy(s.D.host() + w.oD, hd[k], (size_t)2 * w.pnb * sizeof(double));
    }
    double* HG = s.G.host();
    if (ph != PC_BABT)  // the given Gammas (RSQrq reads Gamma_0..N-2, DCtd those of stages with state boxes)
        for (int j = 0; j + 1 < N; j++) {
            const int sd = rup(nxv[j + 1], NCL);
            for (int cc = 0; cc < nxv[j + 1]; cc++)
                for (int i = 0; i < rj[j]; i++) HG[go[j] + i + (long long)cc * rj[j]] = hpGamma[j][idx4(sd, i, cc)];
        }
    if (ph == PC_RSQ) memcpy(R2.host(), pRSQrq2, 8 * nR2);
    if (ph == PC_DCTD) {
        if (nG2) memcpy(G2.host(), pDCt2, 8 * nG2);
        if (nD2) memcpy(D2.host(), d2, 8 * nD2);
    }
    PcArgs a;
    pc_stage(P, s, {blk}, a);
    a.ph = ph | PC_PART;
    a.BAbt2 = B2.dev();
    a.RSQ2 = R2.dev();
    a.DCt2 = G2.dev();
    a.d2 = D2.dev();
    a.idxb2 = I2.dev();
    if (!g_dev.up(c.o) || !launch(WL_PCOND, &a, 1, P.pc_lds, g_dev.stream, "hk_pcond") || !g_dev.down(c.o)) return;
    if (ph == PC_BABT) {  // d_part_cond.c:262-303: Gamma_j (r_j x nx_{j+1}) and BAbt2 = Gamma_{N-1}
        for (int j = 0; j < N; j++) {
            const int sd = rup(nxv[j + 1], NCL);
            for (int cc = 0; cc < nxv[j + 1]; cc++)
                for (int i = 0; i < rj[j]; i++) hpGamma[j][idx4(sd, i, cc)] = HG[go[j] + i + (long long)cc * rj[j]];
        }
        const int sd = rup(nxv[N], NCL);
        for (int cc = 0; cc < nxv[N]; cc++)
            for (int i = 0; i < rj[N - 1]; i++) pBAbt2[idx4(sd, i, cc)] = B2.host()[idx4(sd, i, cc)];
    } else if (ph == PC_RSQ) {
        memcpy(pRSQrq2, R2.host(), 8 * nR2);
    } else {
        if (nG2) memcpy(pDCt2, G2.host(), 8 * nG2);
        if (nD2) memcpy(d2, D2.host(), 8 * nD2);
        if (nbb) memcpy(idxb2, I2.host(), 4 * nbb);
    }
}
}  // namespace

// d_part_cond.c:214-308
extern "C" void d_cond_BAbt(int N, int* nx, int* nu, double** hpBAbt, double* work, double** hpGamma, double* pBAbt2) {
    (void)work;
    cond_part(PC_BABT, N, nx, nu, nullptr, nullptr, hpBAbt, nullptr, nullptr, hpGamma, pBAbt2, nullptr, nullptr,
              nullptr, nullptr);
}

// d_part_cond.c:312-574
extern "C" void d_cond_RSQrq(int N, int* nx, int* nu, double** hpBAbt, double** hpRSQrq, double** hpGamma,
                             double* work, double* pRSQrq2) {
    (void)work;
    cond_part(PC_RSQ, N, nx, nu, nullptr, nullptr, hpBAbt, hpRSQrq, nullptr, hpGamma, nullptr, pRSQrq2, nullptr,
              nullptr, nullptr);
}

// d_part_cond.c:579-689
extern "C" void d_cond_DCtd(int N, int* nx, int* nu, int* nb, int** hidxb, double** hd, double** hpGamma,
                            double* pDCt2, double* d2, int* idxb2) {
    cond_part(PC_DCTD, N, nx, nu, nb, hidxb, nullptr, nullptr, hd, hpGamma, nullptr, nullptr, pDCt2, d2, idxb2);
}

extern "C" int d_part_expand_work_space_size_bytes(int N, int* nx, int* nu, int* nb, int* ng) { return 64; }

// d_part_cond.c:1103-1308
extern "C" void d_part_expand_solution(int N, int* nx, int* nu, int* nb, int** hidxb, int* ng, double** hpBAbt,
                                       double** hb, double** hpRSQrq, double** hrq, double** hpDCt, double** hux,
                                       double** hpi, double** hlam, double** ht, int N2, int* nx2, int* nu2, int* nb2,
                                       int** hidxb2, int* ng2, double** hux2, double** hpi2, double** hlam2,
                                       double** ht2, void* work) {
    (void)work;
    (void)hpDCt;  // only the last stage may carry general constraints (d_part_cond.c:971-976): copied, not used
    (void)hidxb2;
    hk_set_error(0, nullptr);
    PcPlan P;
    if (!pc_plan(P, N, nx, nu, nb, hidxb, ng, N2)) return;
    const WLayout &O = P.orig, &C = P.cond;
    Carve c;
    const Slot<WideStage> St = c.take<WideStage>(N + 1), St2 = c.take<WideStage>(N2 + 1);
    const Slot<PcBlock> Blk = c.take<PcBlock>(N2);
    const Slot<int> Idx = c.take<int>(O.nI);
    const Slot<double> B = c.take<double>(O.nB), R = c.take<double>(O.nR), vb = c.take<double>(O.nP),
                       vrq = c.take<double>(O.nU), U2 = c.take<double>(C.nU), P2 = c.take<double>(C.nP),
                       L2 = c.take<double>(C.nD), T2 = c.take<double>(C.nD), U = c.take<double>(O.nU),
                       Pi = c.take<double>(O.nP), Lam = c.take<double>(O.nD), T = c.take<double>(O.nD);
    if (!g_dev.ensure(c.o)) return;
    St.put(O.st);
    St2.put(C.st);
    Blk.put(P.blk);
    Idx.put(P.idxb);
    BAbt_in(O, B.host(), hpBAbt);
    RSQ_in(O, R.host(), hpRSQrq);
    pvec_in(O, vb.host(), hb);
    uvec_in(O, vrq.host(), hrq);
    uvec_in(C, U2.host(), hux2);
    pvec_in(C, P2.host(), hpi2);
    cvec_in(C, L2.host(), hlam2);
    cvec_in(C, T2.host(), ht2);
    PxArgs a;
    fill_px_args(P, a);
    a.nprob = 1;
    a.st = St.dev();
    a.st2 = St2.dev();
    a.blk = Blk.dev();
    a.idxb = Idx.dev();
    a.BAbt = B.dev();
    a.RSQ = R.dev();
    a.hb = vb.dev();
    a.hrq = vrq.dev();
    a.ux2 = U2.dev();
    a.pi2 = P2.dev();
    a.lam2 = L2.dev();
    a.t2 = T2.dev();
    a.ux = U.dev();
    a.pi = Pi.dev();
    a.lam = Lam.dev();
    a.t = T.dev();
    if (!g_dev.up(c.o) || !launch(WL_PEXPAND, &a, 1, P.px_lds, g_dev.stream, "hk_pexpand") || !g_dev.down(c.o)) return;
    uvec_out(O, U.host(), hux);
    pvec_out(O, Pi.host(), hpi);
    for (int k = 0; k <= N; k++) {
        const WideStage& s = O.st[k];
        // only the slots the reference writes: boxes [0, nb) / [pnb, pnb+nb) and, at N, the generals
        for (int l = 0; l < s.nb; l++) {
            hlam[k][l] = Lam.host()[s.oD + l];
            hlam[k][s.pnb + l] = Lam.host()[s.oD + s.pnb + l];
            ht[k][l] = T.host()[s.oD + l];
            ht[k][s.pnb + l] = T.host()[s.oD + s.pnb + l];
        }
        for (int l = 2 * s.pnb; k == N && l < len_cvec(s); l++) {
            hlam[k][l] = Lam.host()[s.oD + l];
            ht[k][l] = T.host()[s.oD + l];
        }
    }
}

// ------------------------------------------------------------------------------------------------
// Batched device API of the partial-condensing pipeline (data resident in HBM, problem-major).
// ------------------------------------------------------------------------------------------------
struct hpmpc_mi355x_pcond_plan {
    PcPlan P;
    hpmpc_mi355x_wide_plan* wide = nullptr;  // the condensed problem's IPM plan (null: beyond the wide IPM)
    DevTable<WideStage> d_st, d_st2;
    DevTable<PcBlock> d_blk;
    DevTable<int> d_idxb;
    // hk_pcond's blocks of problem 0 write the condensed box indices here: the values pc_plan computed (P.idxb2),
    // which the upload has already put there, so the table is rewritten with what it holds
    DevTable<int> d_idxb2;
    ~hpmpc_mi355x_pcond_plan() { hpmpc_mi355x_wide_plan_destroy(wide); }
};

extern "C" void hpmpc_mi355x_pcond_plan_destroy(hpmpc_mi355x_pcond_plan* q) { delete q; }

extern "C" hpmpc_mi355x_pcond_plan* hpmpc_mi355x_pcond_plan_create(int N, const int* nx, const int* nu, const int* nb,
                                                                   const int* const* idxb, const int* ng, int N2) {
    hk_set_error(0, nullptr);
    auto* q = new hpmpc_mi355x_pcond_plan();
    const PcPlan& P = q->P;
    if (!pc_plan(q->P, N, nx, nu, nb, idxb, ng, N2) || !q->d_st.upload(P.orig.st, "pcond plan") ||
        !q->d_st2.upload(P.cond.st, "pcond plan") || !q->d_blk.upload(P.blk, "pcond plan") ||
        !q->d_idxb.upload(P.idxb, "pcond plan") || !q->d_idxb2.upload(P.idxb2, "pcond plan")) {
        delete q;
        return nullptr;
    }
    // the condensed problem's wide-stage IPM plan (hpmpc_mi355x_pcond_wide_plan); its DCt2 holds the blocks'
    // general constraints only, so a terminal stage with ng[N] > 0 leaves the plan without it
    if (ng[N] == 0) {
        std::vector<int*> i2(N2 + 1);
        for (int k = 0; k <= N2; k++) i2[k] = q->P.idxb2.data() + P.cond.st[k].oI;
        q->wide = hpmpc_mi355x_wide_plan_create(N2, P.nx2.data(), P.nu2.data(), P.nb2.data(), i2.data(),
                                                P.ng2.data());
        // the wide IPM indexes BAbt2 / RSQrq2 / DCt2 / d2 / ux2 / pi2 with its own layout: it must be exactly the
        // condensing kernels' carve (same per-problem sizes, same stage offsets), or it would read other blocks
        if (q->wide) {
            long long ws[8];
            std::vector<long long> wo(6 * (size_t)(N2 + 1));
            bool same = hpmpc_mi355x_wide_sizes(q->wide, ws) == 0 && hpmpc_mi355x_wide_offsets(q->wide, wo.data()) == 0;
            same = same && ws[0] == P.cond.nB && ws[1] == P.cond.nR && ws[2] == P.nG2 && ws[3] == P.cond.nD &&
                   ws[4] == P.cond.nU && ws[5] == P.cond.nP;
            for (int k = 0; same && k <= N2; k++) {
                const WideStage& s2 = P.cond.st[k];
                const long long* o = wo.data() + 6 * k;  // oB, oR, oG, oD, oU, oP
                same = o[0] == s2.oB && o[1] == s2.oR && o[3] == s2.oD && o[4] == s2.oU && o[5] == s2.oP &&
                       (k == N2 || P.ng2[k] == 0 || o[2] == P.blk[k].oG2);
            }
            if (!same) {
                fprintf(stderr, "hpmpc_mi355x: condensed wide IPM layout differs from the condensing carve\n");
                hpmpc_mi355x_wide_plan_destroy(q->wide);
                q->wide = nullptr;
            }
        }
    }
    hk_set_error(0, nullptr);  // a condensed problem beyond the wide IPM keeps the condense / Riccati pipeline
    return q;
}

// The condensed problem's IPM plan (owned by the pcond plan; null when the condensed stages exceed the wide
// IPM's limits or ng[N] > 0): hpmpc_mi355x_wide_ipm_batch on BAbt2 / RSQrq2 / DCt2 / d2 solves the condensed
// problems, hpmpc_mi355x_pexpand_batch expands their solution and multipliers.
extern "C" const hpmpc_mi355x_wide_plan* hpmpc_mi355x_pcond_wide_plan(const hpmpc_mi355x_pcond_plan* q) {
    if (!q || !q->wide) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "no wide IPM plan for this condensed problem");
        return nullptr;
    }
    return q->wide;
}

// Per-problem sizes (doubles): [0] BAbt [1] RSQrq [2] d (=lam/t) [3] ux [4] pi of the original layout;
// [5] BAbt2 [6] RSQrq2 [7] DCt2 [8] d2 [9] ux2 [10] pi2 [11] condensed factor [12] Gamma scratch;
// [13] condensed stages N2, [14] max ng2 (the condensed Riccati needs 0).
extern "C" int hpmpc_mi355x_pcond_sizes(const hpmpc_mi355x_pcond_plan* q, long long* out) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    const PcPlan& P = q->P;
    long long v[15] = {P.orig.nB, P.orig.nR, P.orig.nD, P.orig.nU, P.orig.nP, P.cond.nB, P.cond.nR, P.nG2,
                       P.cond.nD, P.cond.nU, P.cond.nP, P.cond.nL, P.nG, P.N2, 0};
    for (int k = 0; k <= P.N2; k++) v[14] = std::max<long long>(v[14], P.ng2[k]);
    memcpy(out, v, sizeof v);
    return 0;
}

// Stage offsets (doubles) of the layouts, for callers that fill / read the packed arrays:
// which = 0 original, 1 condensed; out[k*6 + 0..5] = oB, oR, oD, oU, oP, oL of stage k.
extern "C" int hpmpc_mi355x_pcond_offsets(const hpmpc_mi355x_pcond_plan* q, int which, long long* out) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    const WLayout& L = which ? q->P.cond : q->P.orig;
    for (int k = 0; k <= L.N; k++) {
        const WideStage& s = L.st[k];
        const long long v[6] = {s.oB, s.oR, s.oD, s.oU, s.oP, s.oL};
        memcpy(out + 6 * k, v, sizeof v);
    }
    return 0;
}

extern "C" int hpmpc_mi355x_pcond_batch(const hpmpc_mi355x_pcond_plan* q, int nprob, int p0, int count,
                                        const double* BAbt, const double* RSQrq, const double* d, double* G,
                                        double* BAbt2, double* RSQrq2, double* DCt2, double* d2, void* stream) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    hk_set_error(0, nullptr);
    if (((uintptr_t)BAbt | (uintptr_t)RSQrq) & 15) {  // hk_pcond copies their lib4 blocks by 16-byte LDS DMA
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "pcond_batch: BAbt / RSQrq must be 16-byte aligned");
        return HPMPC_MI355X_EUNSUPPORTED;
    }
    PcArgs a;
    fill_pc_args(q->P, a);
    a.nprob = nprob;
    a.p0 = p0;
    a.st = q->d_st.get();
    a.blk = q->d_blk.get();
    a.idxb = q->d_idxb.get();
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.d = d;
    a.G = G;
    a.BAbt2 = BAbt2;
    a.RSQ2 = RSQrq2;
    a.DCt2 = DCt2;
    a.d2 = d2;
    a.idxb2 = const_cast<int*>(q->d_idxb2.get());
    if (const char* e = getenv("HK_PCOND_SKIP")) a.skip = atoi(e);  // profiling only
    return launch(WL_PCOND, &a, count, q->P.pc_lds, (hipStream_t)stream, "hk_pcond") ? 0 : HPMPC_MI355X_EHIP;
}

extern "C" int hpmpc_mi355x_pcond_ric_sv_batch(const hpmpc_mi355x_pcond_plan* q, int nprob, int p0, int count,
                                               const double* BAbt2, const double* RSQrq2, double* ws, double* ux2,
                                               double* pi2, int compute_pi, void* stream) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    hk_set_error(0, nullptr);
    const WLayout& C = q->P.cond;
    if (C.any_ng || !C.fits) {
        hk_set_error(HPMPC_MI355X_EUNSUPPORTED, "condensed Riccati with general constraints (state boxes) or "
                                                "beyond the wide-stage tile limits");
        return HPMPC_MI355X_EUNSUPPORTED;
    }
    WideArgs a;
    memset(&a, 0, sizeof a);
    wide_args(C, nprob, p0, a);
    a.st = q->d_st2.get();
    a.BAbt = BAbt2;
    a.RSQ = RSQrq2;
    a.ws = ws;
    a.ux = ux2;
    a.pi = pi2;
    a.compute_pi = compute_pi;
    if (const char* e = getenv("HK_WIDE_SKIP")) a.skip = atoi(e);  // profiling only
    return launch(WL_SV, &a, count, C.lds, (hipStream_t)stream, "hk_wide_sv") ? 0 : HPMPC_MI355X_EHIP;
}

extern "C" int hpmpc_mi355x_pexpand_batch(const hpmpc_mi355x_pcond_plan* q, int nprob, int p0, int count,
                                          const double* BAbt, const double* RSQrq, const double* ux2,
                                          const double* pi2, const double* lam2, const double* t2, double* ux,
                                          double* pi, double* lam, double* t, void* stream) {
    if (!q) return HPMPC_MI355X_EUNSUPPORTED;
    hk_set_error(0, nullptr);
    PxArgs a;
    fill_px_args(q->P, a);
    a.nprob = nprob;
    a.p0 = p0;
    a.st = q->d_st.get();
    a.st2 = q->d_st2.get();
    a.blk = q->d_blk.get();
    a.idxb = q->d_idxb.get();
    a.BAbt = BAbt;
    a.RSQ = RSQrq;
    a.ux2 = ux2;
    a.pi2 = pi2;
    a.lam2 = lam2;
    a.t2 = t2;
    a.ux = ux;
    a.pi = pi;
    a.lam = lam;
    a.t = t;
    return launch(WL_PEXPAND, &a, count, q->P.px_lds, (hipStream_t)stream, "hk_pexpand") ? 0 : HPMPC_MI355X_EHIP;
}

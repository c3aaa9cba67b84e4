/*
 * hpmpc_mi355x.h -- C ABI of libhpmpc_mi355x.so, the MI355X (gfx950) drop-in for HPMPC's
 * Riccati / interior-point hot path.
 *
 * Part 1 re-exports the reference's own low-level entry points with byte-identical prototypes, so
 * that the reference drivers (test_problems/test_d_ip_hard.c, test_d_ric_mpc.c) and the high-level
 * wrappers (interfaces/c/fortran_order_interface.c) relink against this library unchanged.  Each
 * prototype cites the reference declaration it replaces (paths relative to the reference checkout).
 * All data are the reference's lib4 panel-major buffers (bs = 4, ncl = 2) on the HOST; every call
 * runs on the GPU (no CPU fallback).  Workspace / memory contents are private to this library and
 * are sized by this library's *_size_bytes functions.
 *
 * Part 2 is the additive batched API: many independent QPs that share stage sizes, with all data
 * already resident in device memory (HBM).
 *
 * GPU paths (selected per call from the stage sizes):
 *   tile path -- nu[k] + nx[k] <= 16, round_up(nu[k],4) + nx[k] <= 16 and round_up(nb[k],4) + round_up(ng[k],4)
 *     <= 16 for every stage: one wavefront per problem, the stage in MFMA registers;
 *   wide path -- every other problem with nu[k] + nx[k] + 1 <= 128, nx[k] <= 64 and the stage tiles within
 *     64 KiB of LDS (any nb <= nu+nx, any ng): one 256-thread workgroup per problem, stage tiles in LDS; the
 *     IPMs run whole on the device in one launch.
 *   Part 1 serves both; the batched Part 2 takes tile-path plans (plus the partial-condensing pipeline).
 *   Beyond these limits, and for duplicate box indices, calls report HPMPC_MI355X_EUNSUPPORTED.
 * Error reporting: the reference's int entry points keep their codes 0/1/2/-1; this library adds
 *   HPMPC_MI355X_EUNSUPPORTED (-10), HPMPC_MI355X_EHIP (-11) and HPMPC_MI355X_EMW (-20: the one-problem latency
 *   kernel abandoned a solve after an expired hand-over wait between its waves -- a bug, never a data condition;
 *   see hpmpc_mi355x_ipm_solo).  void entry points set the thread-local code returned by
 *   hpmpc_mi355x_last_error() and print one line to stderr; int entry points set it too.
 */
#ifndef HPMPC_MI355X_H_
#define HPMPC_MI355X_H_

#ifdef __cplusplus
extern "C" {
#endif

#define HPMPC_MI355X_EUNSUPPORTED (-10)
#define HPMPC_MI355X_EHIP (-11)
#define HPMPC_MI355X_EMW (-20)
/* Problem queue control block (hpmpc_mi355x_ipm_queue's qctl): ints for n_slots slots, up to
 * HPMPC_MI355X_QUEUE_LANES_MAX lanes. */
#define HPMPC_MI355X_QUEUE_LANES_MAX 4
#define HPMPC_MI355X_QUEUE_CTL_INTS(n_slots) (6 * HPMPC_MI355X_QUEUE_LANES_MAX + 2 + 3 * (n_slots))

/* ================================ Part 1: reference entry points ================================ */

/* include/lqcp_solvers.h:37 (lqcp_solvers/d_back_ric_rec.c:43) */
int d_back_ric_rec_sv_tv_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int *ng);
/* include/lqcp_solvers.h:39 (d_back_ric_rec.c:79) */
int d_back_ric_rec_sv_tv_memory_space_size_bytes(int N, int *nx, int *nu, int *nb, int *ng);
/* include/lqcp_solvers.h:41 (d_back_ric_rec.c:112) -- factorise + solve */
void d_back_ric_rec_sv_tv_res(int N, int *nx, int *nu, int *nb, int **idxb, int *ng, int update_b, double **hpBAbt,
                              double **b, int update_q, double **hpQ, double **q, double **bd, double **hpDCt,
                              double **Qx, double **qx, double **hux, int compute_pi, double **hpi, int compute_Pb,
                              double **hPb, double *memory, double *work);
/* include/lqcp_solvers.h:43 (d_back_ric_rec.c:403) -- factorise */
void d_back_ric_rec_trf_tv_res(int N, int *nx, int *nu, int *nb, int **idxb, int *ng, double **hpBAbt, double **hpQ,
                               double **hpDCt, double **Qx, double **bd, double *memory, double *work);
/* include/lqcp_solvers.h:45 (d_back_ric_rec.c:564) -- solve with the factor left in memory */
void d_back_ric_rec_trs_tv_res(int N, int *nx, int *nu, int *nb, int **idxb, int *ng, double **hpBAbt, double **hb,
                               double **hq, double **hpDCt, double **qx, double **hux, int compute_pi, double **hpi,
                               int compute_Pb, double **hPb, double *memory, double *work);

/* include/mpc_solvers.h:41 (mpc_solvers/d_ip2_res_hard.c:57) */
int d_ip2_res_mpc_hard_tv_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int *ng);
/* include/mpc_solvers.h:42 (d_ip2_res_hard.c:116) */
int d_ip2_res_mpc_hard_tv(int *kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                          double *stat, int N, int *nx, int *nu_N, int *nb, int **idxb, int *ng, double **pBAbt,
                          double **pQ, double **pDCt, double **d, double **ux, int compute_mult, double **pi,
                          double **lam, double **t, double *double_work_memory);
/* include/mpc_solvers.h:44 (d_ip2_res_hard.c:1348) -- k_max Newton steps from (ux0, pi0, lam0, t0), fixed
 * centering target mu0, no exit test on mu; lam0/t0 as [lower(nb) | upper(nb)] */
int d_ip2_res_mpc_hard_tv_single_newton_step(int *kk, int k_max, double mu0, double mu_tol, double alpha_min,
                                             int warm_start, double *stat, int N, int *nx, int *nu_N, int *nb,
                                             int **idxb, int *ng, double **pBAbt, double **pQ, double **pDCt,
                                             double **d, double **ux, int compute_mult, double **pi, double **lam,
                                             double **t, double *double_work_memory, double **ux0, double **pi0,
                                             double **lam0, double **t0);
/* include/mpc_solvers.h:46 (d_ip2_res_hard.c:1922) -- re-solve with the persisted factor/iterate */
void d_kkt_solve_new_rhs_res_mpc_hard_tv(int N, int *nx, int *nu_N, int *nb, int **idxb, int *ng, double **pBAbt,
                                         double **b, double **pQ, double **q, double **pDCt, double **d,
                                         double **ux, int compute_mult, double **pi, double **lam, double **t,
                                         double *double_work_memory);
/* include/mpc_solvers.h:47 (mpc_solvers/c99/d_res_ip_res_hard.c:39) */
void d_res_res_mpc_hard_tv(int N, int *nx, int *nu, int *nb, int **idxb, int *ng, double **hpBAbt, double **hb,
                           double **hpQ, double **hq, double **hux, double **hpDCt, double **hd, double **hpi,
                           double **hlam, double **ht, double *work, double **hrq, double **hrb, double **hrd,
                           double **hrm, double *mu);

/* The alternate IPM of mpc_solvers/d_ip2_hard.c: the phase-1 Mehrotra loop alone, run to mu_tol. */
/* include/mpc_solvers.h:33 (mpc_solvers/d_ip2_hard.c:31) */
int d_ip2_mpc_hard_tv_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int *ng);
/* include/mpc_solvers.h:34 (d_ip2_hard.c:88) */
int d_ip2_mpc_hard_tv(int *kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start, double *stat,
                      int N, int *nx, int *nu, int *nb, int **idxb, int *ng, double **pBAbt, double **pQ,
                      double **pDCt, double **d, double **ux, int compute_mult, double **pi, double **lam, double **t,
                      double *double_work_memory);
/* include/mpc_solvers.h:35 (d_ip2_hard.c:626) -- re-solve on the factor and lam/t that d_ip2_mpc_hard_tv left in
 * the workspace, for new r_A (b), r_H (q) and r_C (bounds) */
void d_kkt_solve_new_rhs_mpc_hard_tv(int N, int *nx, int *nu_N, int *nb, int **idxb, int *ng, double **pBAbt,
                                     double **r_A, double **pQ, double **r_H, double **pDCt, double **r_C,
                                     double **ux, int compute_mult, double **pi, double **lam, double **t,
                                     double *double_work_memory);
/* Soft-constraint IPM (phase-1 Mehrotra loop with slack variables for the ns soft boxes listed after the nb
 * hard ones in idxb; d = [lb | ub | ls | us], lam / t = [lo | up | 4 soft blocks], Z / z slack penalties).
 * include/mpc_solvers.h:69 (mpc_solvers/d_ip2_soft.c:42) */
int d_ip2_mpc_soft_tv_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int *ng, int *ns);
/* include/mpc_solvers.h:70 (d_ip2_soft.c:83).  HPMPC_MI355X_EUNSUPPORTED for ng > 0, nu[N] != 0, and the sizes
 * where the reference itself reads outside BAbt (soft constraints). */
int d_ip2_mpc_soft_tv(int *kk, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start, double *stat,
                      int N, int *nx, int *nu, int *nb, int **idxb, int *ng, int *ns, double **pBAbt, double **pQ,
                      double **Z, double **z, double **pDCt, double **d, double **ux, int compute_mult, double **pi,
                      double **lam, double **t, double *double_work_memory);
/* include/mpc_solvers.h:71 (mpc_solvers/d_res_ip_soft.c:38) -- r_q, r_b, r_d (hard | general | 2 soft blocks),
 * r_z and mu of a soft-constraint iterate, with the reference's indexing (soft constraint i of stage k on
 * ux[idxb[k][nu_k + i]]) and signs; general constraints allowed.  Entries the reference does not write keep the
 * caller's values. */
void d_res_mpc_soft_tv(int N, int *nx, int *nu, int *nb, int **idxb, int *ng, int *ns, double **hpBAbt, double **hpQ,
                       double **hq, double **hZ, double **hz, double **hux, double **hpDCt, double **hd, double **hpi,
                       double **hlam, double **ht, double **hrq, double **hrb, double **hrd, double **hrz, double *mu);
/* include/mpc_solvers.h:36 (mpc_solvers/d_res_ip_hard.c:38) -- r_q, r_b, r_d and mu (no r_m) */
void d_res_mpc_hard_tv(int N, int *nx, int *nu, int *nb, int **idxb, int *ng, double **hpBAbt, double **hb,
                       double **hpQ, double **hq, double **hux, double **hpDCt, double **hd, double **hpi,
                       double **hlam, double **ht, double **hrq, double **hrb, double **hrd, double *mu);

/* Partial condensing: N stages -> N2 blocks, block i keeping [u_{T-1}; ..; u_0; x_0] as its
 * stage variable.  The condensed data are written into `memory` with the reference's own carve, the pointer
 * arrays hpBAbt2 .. hidxb2 are set into it, and the terminal stage aliases the caller's (d_part_cond.c:1052-1056).
 * Stages with nu+nx > 16 (e.g. the condensed nu2+nx2 = 84 of configs[4]) are solved by
 * d_back_ric_rec_sv_tv_res on the wide-stage path. */
/* The three building blocks of one condensing block (horizon N, condensed variable [u_{N-1}; ..; u_0; x_0]), each
 * one hk_pcond launch.  Gamma_j = hpGamma[j] is lib4 with (sum_{i<=j} nu_i + nx_0 + 1) rows, nx_{j+1} columns,
 * panel stride round_up(nx_{j+1}, 2); work is not used (every temporary is on the device).  Only the elements the
 * reference writes are written, except the strict upper triangle of pRSQrq2 (of each u_s x u_s diagonal block
 * and of the first stage's square), which the reference copies from its work matrix: it is left as the caller
 * had it (every consumer reads the lower triangle).  Limits as for d_part_cond (nx <= 63, Gamma rows x nx <= 3072): else no output and
 * hpmpc_mi355x_last_error() = HPMPC_MI355X_EUNSUPPORTED. */
/* include/lqcp_solvers.h:80 (lqcp_solvers/d_part_cond.c:214) -- Gamma_0..Gamma_{N-1} and pBAbt2 = Gamma_{N-1} */
void d_cond_BAbt(int N, int *nx, int *nu, double **hpBAbt, double *work, double **hpGamma, double *pBAbt2);
/* include/lqcp_solvers.h:82 (d_part_cond.c:312) -- the condensed Hessian from the given Gamma_0..Gamma_{N-2} */
void d_cond_RSQrq(int N, int *nx, int *nu, double **hpBAbt, double **hpRSQrq, double **hpGamma, double *work,
                  double *pRSQrq2);
/* include/lqcp_solvers.h:84 (d_part_cond.c:579) -- boxes of stage 0 and input boxes stay boxes (d2 lower/upper
 * at 0 / round_up(nbb,4), idxb2), state boxes of stages 1..N-1 become rows of pDCt2 with bounds at
 * 2 round_up(nbb,4) / + round_up(nbg,4) */
void d_cond_DCtd(int N, int *nx, int *nu, int *nb, int **hidxb, double **hd, double **hpGamma, double *pDCt2,
                 double *d2, int *idxb2);
/* include/lqcp_solvers.h:86 (lqcp_solvers/d_part_cond.c:694) */
void d_part_cond_compute_problem_size(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, int N2, int *nx2,
                                      int *nu2, int *nb2, int *ng2);
/* include/lqcp_solvers.h:88 (d_part_cond.c:743) -- every temporary lives on the device: 64 bytes */
int d_part_cond_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, int N2, int *nx2,
                                      int *nu2, int *nb2, int *ng2);
/* include/lqcp_solvers.h:90 (d_part_cond.c:868) */
int d_part_cond_memory_space_size_bytes(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, int N2, int *nx2,
                                        int *nu2, int *nb2, int *ng2);
/* include/lqcp_solvers.h:92 (d_part_cond.c:926) */
void d_part_cond(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, double **hpBAbt, double **hpRSQrq,
                 double **hpDCt, double **hd, int N2, int *nx2, int *nu2, int *nb2, int **hidxb2, int *ng2,
                 double **hpBAbt2, double **hpRSQrq2, double **hpDCt2, double **hd2, void *memory, void *work);
/* include/lqcp_solvers.h:94 (d_part_cond.c:1066) */
int d_part_expand_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int *ng);
/* include/lqcp_solvers.h:96 (d_part_cond.c:1103) */
void d_part_expand_solution(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, double **hpBAbt, double **hb,
                            double **hpRSQrq, double **hrq, double **hpDCt, double **hux, double **hpi,
                            double **hlam, double **ht, int N2, int *nx2, int *nu2, int *nb2, int **hidxb2,
                            int *ng2, double **hux2, double **hpi2, double **hlam2, double **ht2, void *work);

/* High-level wrappers of include/c_interface.h: dense problem data in column-major
 * (fortran_order_*) or row-major (c_order_*) layout, packed to lib4 on the host, then partial condensing (N2 < N,
 * ng == 0 before stage N) or not, the residual IPM, the expansion and the residual infinity norms
 * inf_norm_res = [max|r_q|, max|r_b|, max|r_d|, mu], all through the entry points above (on the GPU).
 * lam is returned compact as [lam_lb (nb) | lam_ub (nb) | lam_lg (ng) | lam_ug (ng)].  The KKT re-solve wrappers
 * re-use the factor the IPM wrapper left in work0 (full-space solves only). */
/* include/c_interface.h:59 (interfaces/c/c_interface_work_space.c:70) */
int hpmpc_d_ip_ocp_hard_tv_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, int N2);
/* include/c_interface.h:60 (defined by the reference only in interfaces/c/fortran_order_interface_libstr.c:110): the
 * same size for boxes given by count, nbu[k] inputs and nbx[k] states */
int hpmpc_d_ip_ocp_hard_tv_work_space_size_bytes_noidxb(int N, int *nx, int *nu, int *nb, int *nbx, int *nbu, int *ng, int N2);
/* include/c_interface.h:66 (interfaces/c/fortran_order_interface.c:690) -- k_max Newton steps from (ux0, pi0, lam0,
 * t0) with centering target mu0 on the full space; lam and t returned compact like the IPM wrapper's lam */
int fortran_order_d_ip_ocp_hard_tv_single_newton_step(int *kk, int k_max, double mu0, double mu_tol, int N, int *nx, int *nu_N, int *nb, int **hidxb, int *ng, int N2, int warm_start, double **A, double **B, double **b, double **Q, double **S, double **R, double **q, double **r, double **lb, double **ub, double **C, double **D, double **lg, double **ug, double **x, double **u, double **pi, double **lam, double **t, double *inf_norm_res, void *work0, double *stat, double **ux0, double **pi0, double **lam0, double **t0);
/* include/c_interface.h:70 (interfaces/c/c_interface_work_space.c:177) -- the reference's formula over this library's
 * d_ip2_mpc_soft_tv work space */
int hpmpc_d_ip_ocp_soft_tv_work_space_size_bytes(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, int *ns);
/* include/c_interface.h:71 (interfaces/c/fortran_order_interface.c:1442) -- soft-constraint IPM wrapper: idxb / lb /
 * ub list the nb hard boxes then the ns soft ones, Z / z = [lower (ns) | upper (ns)]; full space; lam returned as
 * [lo nb | up nb | lg ng | ug ng | 4 soft blocks of ns].  As the reference's IPM sees it, z is not used (the
 * reference never copies it, :1712-1719); inf_norm_res comes from d_res_mpc_soft_tv called as declared (the
 * reference's call is shifted by one argument, :1880).  Limits of d_ip2_mpc_soft_tv apply. */
int fortran_order_d_ip_ocp_soft_tv(int *kk, int k_max, double mu0, double mu_tol, int N, int *nx, int *nu_N, int *nb,
                                   int **hidxb, int *ng, int *ns, int warm_start, double **A, double **B, double **b,
                                   double **Q, double **S, double **R, double **q, double **r, double **Z, double **z,
                                   double **lb, double **ub, double **C, double **D, double **lg, double **ug,
                                   double **x, double **u, double **pi, double **lam, double *inf_norm_res,
                                   void *work0, double *stat);
/* include/c_interface.h:62 (interfaces/c/c_order_interface.c:53) */
int c_order_d_ip_ocp_hard_tv(int *kk, int k_max, double mu0, double mu_tol, int N, int *nx, int *nu, int *nb,
                             int **hidxb, int *ng, int N2, int warm_start, double **A, double **B, double **b,
                             double **Q, double **S, double **R, double **q, double **r, double **lb, double **ub,
                             double **C, double **D, double **lg, double **ug, double **x, double **u, double **pi,
                             double **lam, double *inf_norm_res, void *work0, double *stat);
/* include/c_interface.h:63 (interfaces/c/c_order_interface.c:692) */
void c_order_d_solve_kkt_new_rhs_ocp_hard_tv(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng, double **A,
                                             double **B, double **b, double **Q, double **S, double **R, double **q,
                                             double **r, double **lb, double **ub, double **C, double **D, double **lg,
                                             double **ug, double **x, double **u, double **pi, double **lam,
                                             double *inf_norm_res, double *work0);
/* include/c_interface.h:65 (interfaces/c/fortran_order_interface.c:53) */
int fortran_order_d_ip_ocp_hard_tv(int *kk, int k_max, double mu0, double mu_tol, int N, int *nx, int *nu, int *nb,
                                   int **hidxb, int *ng, int N2, int warm_start, double **A, double **B, double **b,
                                   double **Q, double **S, double **R, double **q, double **r, double **lb,
                                   double **ub, double **C, double **D, double **lg, double **ug, double **x,
                                   double **u, double **pi, double **lam, double *inf_norm_res, void *work0,
                                   double *stat);
/* include/c_interface.h:67 (interfaces/c/fortran_order_interface.c:1082) */
void fortran_order_d_solve_kkt_new_rhs_ocp_hard_tv(int N, int *nx, int *nu, int *nb, int **hidxb, int *ng,
                                                   double **A, double **B, double **b, double **Q, double **S,
                                                   double **R, double **q, double **r, double **lb, double **ub,
                                                   double **C, double **D, double **lg, double **ug, double **x,
                                                   double **u, double **pi, double **lam, double *inf_norm_res,
                                                   double *work0);

/* Legacy uniform-size wrappers (include/c_interface.h:40-53; interfaces/c/fortran_order_interface.c:1975,3017,
 * c_order_interface.c:1052,2083): N stages of nx states / nu inputs in flat arrays (time_invariant: one copy of each
 * stage array; lg / ug are read per stage either way), x0 = x[0..nx) folded into stage 0, nb boxes per stage
 * ([inputs | states]; nb - nu state boxes on stage N), ng general constraints per stage and ngN on stage N; the
 * alternate IPM d_ip2_mpc_hard_tv, then d_res_mpc_hard_tv for inf_norm_res.  u (N nu), x (stages 1..N), pi (N nx),
 * lam / t with stage stride 2 nb + 2 ng.  The KKT twins re-solve on the factor the IPM wrapper left in work0 with
 * new x0, b, r, q, qf and bounds.  The reference's quirks and the reads it makes of unwritten memory are listed in
 * hpmpc_amd/csrc/hpmpc_capi_mpc.cpp. */
/* include/c_interface.h:40 -- declared, never defined by the reference: the doubles of work0 these wrappers use */
int hpmpc_d_ip_mpc_hard_tv_work_space_size_doubles(int N, int nx, int nu, int nb, int ng, int ngN);
/* include/c_interface.h:45 (interfaces/c/c_order_interface.c:1052) */
int c_order_d_ip_mpc_hard_tv(int *kk, int k_max, double mu0, double mu_tol, int N, int nx, int nu, int nb, int ng,
                             int ngN, int time_invariant, int free_x0, int warm_start, double *A, double *B,
                             double *b, double *Q, double *Qf, double *S, double *R, double *q, double *qf, double *r,
                             double *lb, double *ub, double *C, double *D, double *lg, double *ug, double *Cf,
                             double *lgf, double *ugf, double *x, double *u, double *pi, double *lam, double *t,
                             double *inf_norm_res, double *work0, double *stat);
/* include/c_interface.h:46 (interfaces/c/c_order_interface.c:2083) */
void c_order_d_solve_kkt_new_rhs_mpc_hard_tv(int N, int nx, int nu, int nb, int ng, int ngN, int time_invariant,
                                             int free_x0, double *A, double *B, double *b, double *Q, double *Qf,
                                             double *S, double *R, double *q, double *qf, double *r, double *lb,
                                             double *ub, double *C, double *D, double *lg, double *ug, double *Cf,
                                             double *lgf, double *ugf, double *x, double *u, double *pi, double *lam,
                                             double *t, double *inf_norm_res, double *work0);
/* include/c_interface.h:52 (interfaces/c/fortran_order_interface.c:1975) */
int fortran_order_d_ip_mpc_hard_tv(int *kk, int k_max, double mu0, double mu_tol, int N, int nx, int nu, int nb,
                                   int ng, int ngN, int time_invariant, int free_x0, int warm_start, double *A,
                                   double *B, double *b, double *Q, double *Qf, double *S, double *R, double *q,
                                   double *qf, double *r, double *lb, double *ub, double *C, double *D, double *lg,
                                   double *ug, double *Cf, double *lgf, double *ugf, double *x, double *u, double *pi,
                                   double *lam, double *t, double *inf_norm_res, double *work0, double *stat);
/* include/c_interface.h:53 (interfaces/c/fortran_order_interface.c:3017) */
void fortran_order_d_solve_kkt_new_rhs_mpc_hard_tv(int N, int nx, int nu, int nb, int ng, int ngN, int time_invariant,
                                                   int free_x0, double *A, double *B, double *b, double *Q, double *Qf,
                                                   double *S, double *R, double *q, double *qf, double *r, double *lb,
                                                   double *ub, double *C, double *D, double *lg, double *ug,
                                                   double *Cf, double *lgf, double *ugf, double *x, double *u,
                                                   double *pi, double *lam, double *t, double *inf_norm_res,
                                                   double *work0);

/* ================================ Part 2: batched device API ==================================== */

/* Opaque plan: stage sizes, box indices and device tables shared by every problem of a batch. */
typedef struct hpmpc_mi355x_plan hpmpc_mi355x_plan;

/* Create a plan for horizon N with per-stage sizes (nu[N] is ignored and treated as 0; idxb[k]
 * lists the nb[k] boxed variables of stage k).  Returns NULL on unsupported sizes. */
hpmpc_mi355x_plan *hpmpc_mi355x_plan_create(int N, const int *nx, const int *nu, const int *nb,
                                            const int *const *idxb, const int *ng);
void hpmpc_mi355x_plan_destroy(hpmpc_mi355x_plan *plan);

/* Device-array geometry of a problem-major batch (all sizes in doubles).  Stage k of problem p reads its BAbt
 * block at BAbt + p * BAbt_stride + BAbt_off[k], or -- when BAbt_shared[k] is nonzero -- at BAbt + BAbt_off[k] for
 * every problem (likewise RSQrq).  Shared blocks give the time-invariant / aliased mode of the reference drivers
 * (test_problems/test_d_ip_hard.c:652-662: every inner stage points at one block) across a whole batch: e.g. only
 * stage 0 per problem (its b row carries A x0 + b) and one shared inner block for every other stage.  The offsets
 * must fit in 32 bits.  A plan keeps one device table per distinct layout it has seen (its first use uploads it,
 * synchronously), up to 64: a call with a 65th distinct layout fails with HPMPC_MI355X_EUNSUPPORTED. */
typedef struct {
    long long BAbt_stride;   /* doubles between problems (0: shared by all problems) */
    long long RSQrq_stride;
    const long long *BAbt_off;   /* host array [N]   : lib4 block of stage k inside one problem */
    const long long *RSQrq_off;  /* host array [N+1] */
    const unsigned char *BAbt_shared;   /* host array [N] or NULL (no shared block) */
    const unsigned char *RSQrq_shared;  /* host array [N+1] or NULL */
} hpmpc_mi355x_layout;

/* Doubles of per-problem device workspace the batched calls need (factor + IPM iterate). */
long long hpmpc_mi355x_ws_doubles(const hpmpc_mi355x_plan *plan);

/* Batched d_ip2_res_mpc_hard_tv on problems [p0, p0+count) of a batch of nprob problems.
 * d, lam, t: 32 doubles per stage ([lb(pnb) | ub(pnb)], reference padded layout inside the stride);
 * ux, pi: 16 doubles per stage (ux in the reference variable order, pi over x_{k+1}).
 * kk, ret: per problem; stat: 5*k_max per problem.  Asynchronous on `stream` (hipStream_t). */
int hpmpc_mi355x_ipm_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                           int count, const double *BAbt, const double *RSQrq, const double *d, double *ux, double *pi,
                           double *lam, double *t, double *ws, int k_max, double mu0, double mu_tol, double alpha_min,
                           int warm_start, int compute_mult, int *kk, int *ret, double *stat, void *stream);

/* Latency path: hpmpc_mi355x_ipm_batch with each problem's WHOLE solve in one launch -- one workgroup per problem
 * runs init and every iteration's passes back to back on one CU, so its stage data and factor stay in that XCD's L2
 * and no launch or host poll separates the passes.  For a lone problem or a handful (configs[1]); for throughput
 * over many problems use hpmpc_mi355x_ipm_queue.  Same arguments as hpmpc_mi355x_ipm_batch; the results agree with
 * it to rounding (the four-wave kernel splits each sweep over waves and hipcc contracts a few products
 * differently), with the same kk and ret on every tested problem.  One exception: if a hand-over wait between the
 * kernel's waves expires (~2^22 polls; a bug, never a data condition) the solve stops after that iteration with
 * ret[p] = HPMPC_MI355X_EMW and stat[5 k_max p + 0..3] = diagnostic integers (flag, expected, found, wave); the
 * reference-named entry points then return HPMPC_MI355X_EMW, set hpmpc_mi355x_last_error() and copy nothing. */
int hpmpc_mi355x_ipm_solo(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0, int count,
                          const double *BAbt, const double *RSQrq, const double *d, double *ux, double *pi,
                          double *lam, double *t, double *ws, int k_max, double mu0, double mu_tol, double alpha_min,
                          int warm_start, int compute_mult, int *kk, int *ret, double *stat, void *stream);

/* One pass of the batched IPM, for callers that interleave their own work or timing: the batched
 * solve above is pass 0 (init) followed by k_max rounds of passes 1 (factorisation), 2 (predictor
 * solve + step length + mu_aff), 3 (corrector solve + step length), 4 (update + residuals); problems
 * that have finished return immediately.  Same arguments as hpmpc_mi355x_ipm_batch plus `pass`. */
int hpmpc_mi355x_ipm_pass(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                          int count, const double *BAbt, const double *RSQrq, const double *d, double *ux, double *pi,
                          double *lam, double *t, double *ws, int k_max, double mu0, double mu_tol, double alpha_min,
                          int warm_start, int compute_mult, int *kk, int *ret, double *stat, int pass, void *stream);

/* hpmpc_mi355x_ipm_batch with a hipEvent pair around every pass kernel; synchronises `stream` and
 * returns in pass_ms[0..4] the summed device time of passes 0..4 (benchmark / profiling use). */
int hpmpc_mi355x_ipm_batch_profiled(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob,
                                    int p0, int count, const double *BAbt, const double *RSQrq, const double *d,
                                    double *ux, double *pi, double *lam, double *t, double *ws, int k_max, double mu0,
                                    double mu_tol, double alpha_min, int warm_start, int compute_mult, int *kk,
                                    int *ret, double *stat, double *pass_ms, void *stream);

/* Problem queue (continuous batching): solve nq problems with n_slots resident solver slots.  Queue
 * entry q solves data problem q % nprob (BAbt/RSQrq/d as in hpmpc_mi355x_ipm_batch, nprob problems);
 * ux/pi/lam/t/kk/ret/stat are per queue entry (nq of each, same strides); ws holds n_slots
 * workspaces; qctl is device scratch of HPMPC_MI355X_QUEUE_CTL_INTS(n_slots) ints.  A slot whose problem has
 * finished takes the next entry at the following iteration, so the GPU is not left idle behind the slowest
 * problem of a batch.  Lanes: the slots are split into L contiguous lanes (HPMPC_MI355X_QUEUE_LANES, environment,
 * default 4, at most one per 1024 slots and HPMPC_MI355X_QUEUE_LANES_MAX), each a queue on its own stream (lane 0
 * on `stream`, the others forked from it and joined back into it) handing out entries from one shared counter
 * (qctl[0]), so that one lane's pass kernels fill the tail of another's.  Lane i's control block starts at
 * qctl[6 i + 3 s_i] (s_i: its first slot): [0] (lane 0: the shared counter of entries handed out), [1] entries
 * the lane finished, [2 + s] the entry its slot s holds (-1 none), then the lengths and entries of two lists of
 * the slots that iterate (workgroup i of an iteration runs the i-th listed slot, so a draining queue keeps one
 * slot per SIMD).  qctl[6 HPMPC_MI355X_QUEUE_LANES_MAX + 3 n_slots] and the
 * next int hold the iterations / problems the drain finished.  Drain: once a lane has handed out every entry and
 * at most its share (by slots) of HPMPC_MI355X_QUEUE_DRAIN (environment, default 768) slots still iterate, its
 * survivors finish one per four-wave workgroup (the multi-wave body of hpmpc_mi355x_ipm_solo) in one launch.  Results are those of hpmpc_mi355x_ipm_batch on each entry: bitwise
 * for the entries finished by the iteration passes (all of them with HPMPC_MI355X_QUEUE_DRAIN=0), to rounding
 * for those finished in the drain (the multi-wave bodies contract a few products differently).  The per-slot
 * workspace is reused, so a queue solve leaves no factor behind for d_kkt_solve_new_rhs_res_mpc_hard_tv; for
 * the same reason its update pass writes neither the iterate backups nor r_m, which only that re-solve reads.
 * Synchronises with the device once per chunk of iterations (it polls the finished counter); on
 * return the last chunk may still be running on `stream`.  An iteration (tick) is three launches: the
 * factorisation, the predictor and corrector of each problem back to back, and the update.  pass_ms (nullable):
 * device time of [init + drain, fact, pred + corr, 0, update] summed over the run and the lanes (the lanes'
 * kernels overlap); n_ticks (nullable): iterations enqueued, summed over the lanes (launches of each kernel). */
int hpmpc_mi355x_ipm_queue(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int nq,
                           int n_slots, const double *BAbt, const double *RSQrq, const double *d, double *ux,
                           double *pi, double *lam, double *t, double *ws, int *qctl, int k_max, double mu0,
                           double mu_tol, double alpha_min, int warm_start, int compute_mult, int *kk, int *ret,
                           double *stat, double *pass_ms, int *n_ticks, void *stream);

/* Batched d_back_ric_rec_sv_tv_res (no box / no update rows): factor into ws, ux/pi as above. */
int hpmpc_mi355x_ric_sv_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                              int count, const double *BAbt, const double *RSQrq, double *ux, double *pi, double *ws,
                              int compute_pi, int compute_Pb, double *Pb, void *stream);

/* Batched d_back_ric_rec_trf_tv_res (factorisation only, no box terms) into ws. */
int hpmpc_mi355x_ric_trf_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                               int count, const double *BAbt, const double *RSQrq, double *ws, void *stream);

/* Batched d_back_ric_rec_trs_tv_res re-using the factor in ws; b (16/stage, state order), q (16/stage,
 * variable order). */
int hpmpc_mi355x_ric_trs_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                               int count, const double *BAbt, const double *RSQrq, const double *b, const double *q,
                               double *ux, double *pi, double *ws, int compute_pi, int compute_Pb, double *Pb,
                               void *stream);

/* Thread-local status of the last call (0 = success). */
int hpmpc_mi355x_last_error(void);
/* Library build string (architecture, kernel variant). */
const char *hpmpc_mi355x_version(void);


/* ---- partial-condensing pipeline on device-resident batches (configs[4]) ----
 * A pcond plan holds the original and the condensed stage layouts shared by a batch.  Arrays are
 * problem-major with the per-problem sizes of hpmpc_mi355x_pcond_sizes and the stage offsets of
 * hpmpc_mi355x_pcond_offsets (lib4 blocks / padded vectors at those offsets). */
typedef struct hpmpc_mi355x_pcond_plan hpmpc_mi355x_pcond_plan;
hpmpc_mi355x_pcond_plan *hpmpc_mi355x_pcond_plan_create(int N, const int *nx, const int *nu, const int *nb,
                                                        const int *const *idxb, const int *ng, int N2);
void hpmpc_mi355x_pcond_plan_destroy(hpmpc_mi355x_pcond_plan *plan);
/* out[15]: original BAbt, RSQrq, d, ux, pi | condensed BAbt2, RSQrq2, DCt2, d2, ux2, pi2, factor | Gamma
 * scratch | N2 | max ng2 (doubles per problem) */
int hpmpc_mi355x_pcond_sizes(const hpmpc_mi355x_pcond_plan *plan, long long *out);
/* out[6*(N+1)] (which 0: original) or out[6*(N2+1)] (which 1: condensed): oB, oR, oD, oU, oP, oL per stage */
int hpmpc_mi355x_pcond_offsets(const hpmpc_mi355x_pcond_plan *plan, int which, long long *out);
/* d_part_cond of problems [p0, p0+count): one workgroup per (block, problem); G is the Gamma scratch */
int hpmpc_mi355x_pcond_batch(const hpmpc_mi355x_pcond_plan *plan, int nprob, int p0, int count, const double *BAbt,
                             const double *RSQrq, const double *d, double *G, double *BAbt2, double *RSQrq2,
                             double *DCt2, double *d2, void *stream);
/* d_back_ric_rec_sv_tv_res on the condensed problems (wide stages; no constraints) */
int hpmpc_mi355x_pcond_ric_sv_batch(const hpmpc_mi355x_pcond_plan *plan, int nprob, int p0, int count,
                                    const double *BAbt2, const double *RSQrq2, double *ws, double *ux2, double *pi2,
                                    int compute_pi, void *stream);
/* d_part_expand_solution (b / rq read from the augmented rows of BAbt / RSQrq) */
int hpmpc_mi355x_pexpand_batch(const hpmpc_mi355x_pcond_plan *plan, int nprob, int p0, int count, const double *BAbt,
                               const double *RSQrq, const double *ux2, const double *pi2, const double *lam2,
                               const double *t2, double *ux, double *pi, double *lam, double *t, void *stream);

/* ---- the IPM on wide stages for device-resident batches ----
 * d_ip2_res_mpc_hard_tv (mpc_solvers/d_ip2_res_hard.c:116) for problems whose stages exceed the 16-wide tile
 * (nu+nx+1 <= 128, nx <= 64, stage tiles within 64 KiB of LDS; any nb <= nu+nx, any ng): one 256-thread
 * workgroup runs a whole solve, one launch per batch.  Arrays are problem-major with the per-problem sizes of
 * hpmpc_mi355x_wide_sizes and the stage offsets of hpmpc_mi355x_wide_offsets; the lib4 blocks, the padded
 * [lb | ub | lg | ug] vectors and the DCt blocks sit at those offsets. */
typedef struct hpmpc_mi355x_wide_plan hpmpc_mi355x_wide_plan;
hpmpc_mi355x_wide_plan *hpmpc_mi355x_wide_plan_create(int N, const int *nx, const int *nu, const int *nb,
                                                      const int *const *idxb, const int *ng);
void hpmpc_mi355x_wide_plan_destroy(hpmpc_mi355x_wide_plan *plan);
/* out[8]: doubles per problem of BAbt, RSQrq, DCt, d (= lam = t), ux, pi, the work image; N */
int hpmpc_mi355x_wide_sizes(const hpmpc_mi355x_wide_plan *plan, long long *out);
/* out[6*(N+1)]: oB, oR, oG, oD, oU, oP per stage */
int hpmpc_mi355x_wide_offsets(const hpmpc_mi355x_wide_plan *plan, long long *out);
/* problems [p0, p0+count) of the batch; kk / ret per problem, stat 5*k_max per problem (nullable), work: each
 * problem's work image (factor, iterate backup).  Every other array is required (DCt only when some stage has
 * ng > 0): a null one returns HPMPC_MI355X_EUNSUPPORTED.  Asynchronous on `stream` (a hipStream_t, or null). */
int hpmpc_mi355x_wide_ipm_batch(const hpmpc_mi355x_wide_plan *plan, int nprob, int p0, int count, const double *BAbt,
                                const double *RSQrq, const double *DCt, const double *d, double *ux, double *pi,
                                double *lam, double *t, double *work, int k_max, double mu0, double mu_tol,
                                double alpha_min, int warm_start, int compute_mult, int *kk, int *ret, double *stat,
                                void *stream);
/* the condensed problem's wide plan of a pcond plan (owned by it; null when ng[N] > 0 or beyond the limits):
 * condense -> hpmpc_mi355x_wide_ipm_batch on BAbt2 / RSQrq2 / DCt2 / d2 -> hpmpc_mi355x_pexpand_batch is the
 * IPM on a partially condensed batch (the c_interface wrappers' N2 < N path, batched) */
const hpmpc_mi355x_wide_plan *hpmpc_mi355x_pcond_wide_plan(const hpmpc_mi355x_pcond_plan *plan);

/* ---- the soft-constraint IPM for device-resident batches ----
 * d_ip2_mpc_soft_tv (mpc_solvers/d_ip2_soft.c:83) on a batch of problems that share stage sizes and box indices and
 * whose arrays are already in HBM: one wavefront per problem runs every iteration (Hessian update, Riccati
 * factorisation and solve, predictor, Riccati solve, corrector) in ONE launch after a short init launch, with no
 * host poll; a problem that meets its exit test retires its wavefront.  The arithmetic is the reference-named
 * entry point's (the same device routines), fused: results agree with it to rounding, with the same kk and ret on
 * every tested problem.
 * Plan: idxb[k] lists the nb[k] hard boxes, then the ns[k] soft ones.  Refused (NULL, hpmpc_mi355x_last_error() =
 * HPMPC_MI355X_EUNSUPPORTED) exactly where d_ip2_mpc_soft_tv is: ng > 0, nu[N] != 0, a b_k the reference reads outside
 * BAbt_k, a stray soft-gradient write into a live Zl, round_up(nb + ns, 4) > 16, stages beyond the 16-wide tile.
 * Arrays (device pointers, problem-major, per-problem sizes from hpmpc_mi355x_soft_sizes, stage offsets from
 * hpmpc_mi355x_soft_offsets), each stage in the reference's layout:
 *   d      [lb pnb | ub pnb | ls pns | us pns] at oD[k]       Z, z   [lower pns | upper pns] at oZ[k]
 *   lam, t [lo pnb | up pnb | 4 x pns] at oC[k]               ux, pi 16 doubles per stage (as hpmpc_mi355x_ipm_batch)
 * BAbt / RSQrq follow `lay` as in hpmpc_mi355x_ipm_batch (NULL: the packed default; shared blocks allowed).  ws: the
 * per-problem workspace (factor, step vectors, dt / dlam / lamt / tinv, the reference's flat Qx | qx | Zl | zl block,
 * loop state); it needs no initialisation.  kk, ret per problem; stat 5*k_max per problem.  Only problems
 * [p0, p0+count) are read or written.  Asynchronous on `stream`; nothing in the call synchronises with the device
 * (the first use of a layout uploads its stage table, as for every batched call).  With no constraint on any stage
 * kk[p] = 0, ret[p] = 0 and nothing else is written, as in the reference (d_ip2_soft.c:273-284). */
typedef struct hpmpc_mi355x_soft_plan hpmpc_mi355x_soft_plan;
hpmpc_mi355x_soft_plan *hpmpc_mi355x_soft_plan_create(int N, const int *nx, const int *nu, const int *nb,
                                                      const int *const *idxb, const int *ng, const int *ns);
void hpmpc_mi355x_soft_plan_destroy(hpmpc_mi355x_soft_plan *plan);
/* out[6]: doubles per problem of d, Z (= z), lam (= t), ux (= pi), ws; N */
int hpmpc_mi355x_soft_sizes(const hpmpc_mi355x_soft_plan *plan, long long *out);
/* out[3*(N+1)]: oD, oZ, oC per stage */
int hpmpc_mi355x_soft_offsets(const hpmpc_mi355x_soft_plan *plan, long long *out);
int hpmpc_mi355x_ipm_soft_batch(const hpmpc_mi355x_soft_plan *plan, const hpmpc_mi355x_layout *lay, int nprob,
                                int p0, int count, const double *BAbt, const double *RSQrq, const double *Z,
                                const double *z, const double *d, double *ux, double *pi, double *lam, double *t,
                                double *ws, int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                                int compute_mult, int *kk, int *ret, double *stat, void *stream);

/* ---- the OCP front end for device-resident batches ----
 * The top layer of the include/c_interface.h wrappers (fortran_order_d_ip_ocp_hard_tv / c_order_d_ip_ocp_hard_tv)
 * for a batch of problems that share stage sizes and box indices and whose DENSE data are already in HBM: pack to
 * lib4 on the device, solve, and unpack to the wrappers' outputs, with no host copy in between.
 *   hpmpc_mi355x_ocp_pack_batch   dense A, B, b, Q, S, R, q, r, lb, ub, C, D, lg, ug -> BAbt, RSQrq, DCt, d (ux)
 *   hpmpc_mi355x_ocp_ipm_batch    d_ip2_res_mpc_hard_tv on the packed arrays, general constraints included
 *   hpmpc_mi355x_ocp_finish_batch u, x (with the equality-box fix), pi, compact lam / t, inf_norm_res
 * Tile-path sizes only (see the top of this file), and the full space only: there is no N2; partially condensed
 * batches go through the hpmpc_mi355x_pcond_* pipeline.  Every other Part-2 call (hpmpc_mi355x_ipm_batch, _solo,
 * _pass, _queue, the ric_*_batch calls) still refuses a plan with ng > 0: they carry no DCt array
 * (hpmpc_mi355x_kkt_new_rhs_batch below does, and takes such a plan).
 *
 * Dense arrays (device pointers, doubles).  Inside one problem the stage blocks are concatenated in stage order:
 *   A_k (nx[k+1] x nx[k]), B_k (nx[k+1] x nu[k]), b_k (nx[k+1])        k < N
 *   Q_k (nx[k] x nx[k]), q_k (nx[k])                                   k <= N
 *   S_k (nu[k] x nx[k]), R_k (nu[k] x nu[k]), r_k (nu[k])              k < N
 *   lb_k, ub_k (nb[k]); C_k (ng[k] x nx[k]), lg_k, ug_k (ng[k])        k <= N;     D_k (ng[k] x nu[k])  k < N
 * each matrix block column-major (row_major = 0, the fortran_order_ convention) or row-major (row_major = 1, the
 * c_order_ convention).  Every array has its own problem stride; stride 0 means one copy shared by every problem
 * (time-invariant data).  An array whose per-problem size is 0 (C, D, lg, ug without general constraints; lb, ub
 * without boxes) may be null.
 * Packed arrays: problem-major, per-problem sizes from hpmpc_mi355x_ocp_sizes, in the tile plan's packed default
 * layout (BAbt_k / RSQrq_k / DCt_k at the offsets hpmpc_mi355x_ocp_offsets reports; d, lam, t 32 doubles per stage
 * as [lb pnb | ub pnb | lg png | ug png]; ux, pi 16 doubles per stage) -- with ng = 0 they can be handed, with
 * hpmpc_mi355x_ocp_tile_plan's plan and a null layout, to hpmpc_mi355x_ipm_batch / _solo / _queue.
 * Outputs: u, x, pi shaped like r, q, b; lam, t per stage compact as [lb nb | ub nb | lg ng | ug ng], stages
 * concatenated; inf_norm_res 4 doubles per problem = max|r_q|, max|r_b|, max|r_d|, mu of d_res_mpc_hard_tv, over
 * the elements the one-problem wrappers visit.
 * All calls are asynchronous on `stream` (a hipStream_t, or null) and synchronise with nothing (plan creation
 * uploads its tables once); only problems [p0, p0+count) are read or written; count = 0 returns 0 and does
 * nothing; a null required pointer, a bad range or a refused launch returns HPMPC_MI355X_EUNSUPPORTED. */
typedef struct hpmpc_mi355x_ocp_plan hpmpc_mi355x_ocp_plan;
/* index of each dense array in hpmpc_mi355x_ocp_data, hpmpc_mi355x_ocp_sizes and hpmpc_mi355x_ocp_offsets */
enum {
    HPMPC_MI355X_OCP_A, HPMPC_MI355X_OCP_B, HPMPC_MI355X_OCP_b, HPMPC_MI355X_OCP_Q, HPMPC_MI355X_OCP_S,
    HPMPC_MI355X_OCP_R, HPMPC_MI355X_OCP_q, HPMPC_MI355X_OCP_r, HPMPC_MI355X_OCP_lb, HPMPC_MI355X_OCP_ub,
    HPMPC_MI355X_OCP_C, HPMPC_MI355X_OCP_D, HPMPC_MI355X_OCP_lg, HPMPC_MI355X_OCP_ug, HPMPC_MI355X_OCP_NARRAYS
};
typedef struct {
    const double *ptr[HPMPC_MI355X_OCP_NARRAYS];  /* device pointers: A, B, b, Q, S, R, q, r, lb, ub, C, D, lg, ug */
    long long stride[HPMPC_MI355X_OCP_NARRAYS];   /* doubles between problems (0: shared by all problems) */
} hpmpc_mi355x_ocp_data;
/* nu has N+1 entries (nu[N] is treated as 0); idxb[k] lists the nb[k] boxed variables of stage k.  NULL with
 * hpmpc_mi355x_last_error() = HPMPC_MI355X_EUNSUPPORTED where hpmpc_mi355x_plan_create refuses, and for
 * nb[k] > nu[k] + nx[k]. */
hpmpc_mi355x_ocp_plan *hpmpc_mi355x_ocp_plan_create(int N, const int *nx, const int *nu, const int *nb,
                                                    const int *const *idxb, const int *ng, int row_major);
void hpmpc_mi355x_ocp_plan_destroy(hpmpc_mi355x_ocp_plan *plan);
/* the tile plan the packed arrays belong to (owned by the OCP plan) */
const hpmpc_mi355x_plan *hpmpc_mi355x_ocp_tile_plan(const hpmpc_mi355x_ocp_plan *plan);
/* out[HPMPC_MI355X_OCP_NSIZES], doubles per problem: [0..13] the dense arrays (order above) | [14] BAbt, [15] RSQrq,
 * [16] DCt, [17] d, [18] ux, [19] pi, [20] lam (= t), [21] ws, [22] the residual scratch of
 * hpmpc_mi355x_ocp_finish_batch | outputs [23] u (= u0), [24] x (= x0), [25] pi, [26] lam (= t), [27] inf_norm_res |
 * [28] N */
#define HPMPC_MI355X_OCP_NSIZES 29
int hpmpc_mi355x_ocp_sizes(const hpmpc_mi355x_ocp_plan *plan, long long *out);
/* out[HPMPC_MI355X_OCP_NOFFSETS * (N+1)], per stage: [0..13] the stage's block inside one problem of each dense
 * array (the u / x / pi outputs sit at the offsets of r / q / b), [14] its lam / t output, [15] BAbt_k, [16] RSQrq_k,
 * [17] DCt_k inside the packed arrays */
#define HPMPC_MI355X_OCP_NOFFSETS 18
int hpmpc_mi355x_ocp_offsets(const hpmpc_mi355x_ocp_plan *plan, long long *out);
/* Dense -> packed, exactly the elements oracle/iface_oracle.py to_qp builds (the one-problem wrappers' packing,
 * with S in both triangles of RSQrq_k).  matrices != 0 writes EVERY element of BAbt, RSQrq, DCt and d of the
 * problems in range, padding as zeros: the buffers need no initialisation.  matrices = 0 rewrites only the b row of
 * BAbt_k, the r / q row of RSQrq_k and d (the KKT wrappers' re-pack; the per-step update of a receding-horizon
 * loop) and leaves every other element as it was.  u0, x0, ux: all three given, ux_k = [u0_k | x0_k | 0..] is
 * written for warm_start = 1 (u0 / x0 shaped like the u / x outputs); else ux is not touched.  DCt may be null when
 * every ng is 0. */
int hpmpc_mi355x_ocp_pack_batch(const hpmpc_mi355x_ocp_plan *plan, const hpmpc_mi355x_ocp_data *data, int matrices,
                                int nprob, int p0, int count, double *BAbt, double *RSQrq, double *DCt, double *d,
                                const double *u0, const double *x0, double *ux, void *stream);
/* hpmpc_mi355x_ipm_batch (the same pass kernels: init, then k_max x (factorisation, predictor, corrector, update))
 * on the packed default layout, plus DCt (null when every ng is 0).  kk, ret per problem, stat 5*k_max per problem;
 * ws: hpmpc_mi355x_ocp_sizes()[21] doubles per problem (= hpmpc_mi355x_ws_doubles of the tile plan).  mu0 must be > 0
 * (HPMPC_MI355X_EUNSUPPORTED otherwise): the one-problem wrappers replace mu0 <= 0 by the problem's largest cost
 * entry, a per-problem value, and the batched kernels take one mu0 for the whole batch. */
int hpmpc_mi355x_ocp_ipm_batch(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, const double *BAbt,
                               const double *RSQrq, const double *DCt, const double *d, double *ux, double *pi,
                               double *lam, double *t, double *ws, int k_max, double mu0, double mu_tol,
                               double alpha_min, int warm_start, int compute_mult, int *kk, int *ret, double *stat,
                               void *stream);
/* The wrappers' outputs from the iterate: the plain residuals d_res_mpc_hard_tv over the batch into `res` (nprob *
 * hpmpc_mi355x_ocp_sizes()[22] doubles, no initialisation needed; ws and its factor are not touched), then u, x,
 * pi_out, lam_out, inf_norm_res and, when t_out is not null, t_out. */
int hpmpc_mi355x_ocp_finish_batch(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, const double *BAbt,
                                  const double *RSQrq, const double *DCt, const double *d, const double *ux,
                                  const double *pi, const double *lam, const double *t, double *res, double *u,
                                  double *x, double *pi_out, double *lam_out, double *t_out, double *inf_norm_res,
                                  void *stream);

/* ---- the OCP front end for device-resident batches of SOFT-constrained problems ----
 * The top layer of fortran_order_d_ip_ocp_soft_tv for a batch of problems that share stage sizes and box indices and
 * whose DENSE data are already in HBM: pack on the device, solve with hpmpc_mi355x_ipm_soft_batch's kernel, and unpack
 * to the wrapper's outputs and residual norms, with no host copy in between.
 *   hpmpc_mi355x_ocp_soft_pack_batch   dense A, B, b, Q, S, R, q, r, lb, ub, Z, z -> BAbt, RSQrq, d, Z, z (ux)
 *   hpmpc_mi355x_ocp_soft_ipm_batch    d_ip2_mpc_soft_tv on the packed arrays, every iteration in one launch
 *   hpmpc_mi355x_ocp_soft_finish_batch u, x, pi, compact lam / t, inf_norm_res of d_res_mpc_soft_tv
 * The conventions are those of the hpmpc_mi355x_ocp_* block above: asynchronous on `stream`, no synchronisation, only
 * problems [p0, p0+count) read or written, count = 0 returns 0, a null required pointer or a bad range returns
 * HPMPC_MI355X_EUNSUPPORTED.
 * Dense arrays: as in the block above (A_k .. r_k), with idxb[k] / lb_k / ub_k listing the nb[k] hard boxes, then the
 * ns[k] soft ones (nb[k] + ns[k] entries per stage), and Z_k / z_k (2 ns[k]) = [lower ns | upper ns] the quadratic /
 * linear slack penalties.
 * Packed arrays: exactly what hpmpc_mi355x_ipm_soft_batch takes with hpmpc_mi355x_ocp_soft_ipm_plan's plan and a
 * null layout; their per-problem sizes equal hpmpc_mi355x_soft_sizes' on that plan.  Placement is that of
 * oracle/iface_oracle.py to_soft_qp: BAbt / RSQrq as hpmpc_mi355x_ocp_pack_batch builds them (S in both triangles),
 * d_k = [lb pnb | ub pnb | ls pns | us pns] with the soft bounds read at lb_k[nb + i] / ub_k[nb + i], Z_k padded to
 * pns per half.
 * THE LINEAR PENALTY z.  The reference wrapper never copies z into the IPM (fortran_order_interface.c:1712-1719), and
 * neither does fortran_order_d_ip_ocp_soft_tv here: both solve with z = 0.  In this block a NULL dense z packs zeros
 * -- the reference wrapper's behaviour -- and a GIVEN z is packed like Z and used by the solve and the residual: a
 * documented extension.
 * res_ok.  The reference's soft residual reads the variable of soft constraint i of stage k at idxb[k][nu[k] + i]
 * (d_res_ip_soft.c:107), not at idxb[k][nb[k] + i].  That read stays inside the nb[k] + ns[k] entries only if every
 * stage k < N with ns[k] > 0 has nu[k] <= nb[k]; the plan records this as res_ok (1, else 0).  On a plan with
 * res_ok = 0 the residual norms are refused (HPMPC_MI355X_EUNSUPPORTED, nothing launched); the finish without norms
 * works on every plan.
 * Outputs: u, x, pi shaped like r, q, b; lam, t per stage compact as [lo nb | up nb | 4 soft blocks of ns] (the
 * wrapper's layout with ng = 0); inf_norm_res 4 doubles per problem = max|r_q|, max|r_b|, max|r_d|, mu over the
 * elements the one-problem wrapper visits (maxima from 0). */
typedef struct hpmpc_mi355x_ocp_soft_plan hpmpc_mi355x_ocp_soft_plan;
/* index of each dense array in hpmpc_mi355x_ocp_soft_data, hpmpc_mi355x_ocp_soft_sizes and _offsets: the first ten
 * are HPMPC_MI355X_OCP_A .. HPMPC_MI355X_OCP_ub */
enum { HPMPC_MI355X_OCP_SOFT_Z = 10, HPMPC_MI355X_OCP_SOFT_z = 11, HPMPC_MI355X_OCP_SOFT_NARRAYS = 12 };
typedef struct {
    const double *ptr[HPMPC_MI355X_OCP_SOFT_NARRAYS];  /* device pointers: A, B, b, Q, S, R, q, r, lb, ub, Z, z */
    long long stride[HPMPC_MI355X_OCP_SOFT_NARRAYS];   /* doubles between problems (0: shared by all problems) */
} hpmpc_mi355x_ocp_soft_data;
/* nu has N+1 entries (nu[N] is treated as 0).  NULL with hpmpc_mi355x_last_error() = HPMPC_MI355X_EUNSUPPORTED
 * exactly where hpmpc_mi355x_soft_plan_create refuses (ng > 0 among them), and for nb[k] + ns[k] > nu[k] + nx[k]. */
hpmpc_mi355x_ocp_soft_plan *hpmpc_mi355x_ocp_soft_plan_create(int N, const int *nx, const int *nu, const int *nb,
                                                              const int *const *idxb, const int *ng, const int *ns,
                                                              int row_major);
void hpmpc_mi355x_ocp_soft_plan_destroy(hpmpc_mi355x_ocp_soft_plan *plan);
/* the soft plan the packed arrays belong to (owned by the soft OCP plan) */
const hpmpc_mi355x_soft_plan *hpmpc_mi355x_ocp_soft_ipm_plan(const hpmpc_mi355x_ocp_soft_plan *plan);
/* out[HPMPC_MI355X_OCP_SOFT_NSIZES], doubles per problem: [0..11] the dense arrays (order above) | packed [12] BAbt,
 * [13] RSQrq, [14] d, [15] Z (= z), [16] ux (= pi), [17] lam (= t), [18] ws | [19] the residual scratch of
 * hpmpc_mi355x_ocp_soft_finish_batch | outputs [20] u (= u0), [21] x (= x0), [22] pi, [23] lam (= t),
 * [24] inf_norm_res | [25] res_ok | [26] N */
#define HPMPC_MI355X_OCP_SOFT_NSIZES 27
int hpmpc_mi355x_ocp_soft_sizes(const hpmpc_mi355x_ocp_soft_plan *plan, long long *out);
/* out[HPMPC_MI355X_OCP_SOFT_NOFFSETS * (N+1)], per stage: [0..11] the stage's block inside one problem of each dense
 * array (the u / x / pi outputs sit at the offsets of r / q / b), [12] its lam / t output, [13] BAbt_k, [14] RSQrq_k,
 * [15] d_k, [16] Z_k (= z_k), [17] lam_k (= t_k) inside the packed arrays */
#define HPMPC_MI355X_OCP_SOFT_NOFFSETS 18
int hpmpc_mi355x_ocp_soft_offsets(const hpmpc_mi355x_ocp_soft_plan *plan, long long *out);
/* Dense -> packed.  matrices != 0 writes EVERY element of BAbt, RSQrq, d, Z and z of the problems in range, padding
 * as zeros: the buffers need no initialisation.  matrices = 0 rewrites only the b row of BAbt_k, the r / q row of
 * RSQrq_k, d, Z and z (the per-step update of a receding-horizon loop).  data->ptr[HPMPC_MI355X_OCP_SOFT_z] may be
 * null: z packs as zeros (see above).  u0, x0, ux: all three given, ux_k = [u0_k | x0_k | 0..] is written for
 * warm_start = 1; else ux is not touched. */
int hpmpc_mi355x_ocp_soft_pack_batch(const hpmpc_mi355x_ocp_soft_plan *plan, const hpmpc_mi355x_ocp_soft_data *data,
                                     int matrices, int nprob, int p0, int count, double *BAbt, double *RSQrq,
                                     double *d, double *Z, double *z, const double *u0, const double *x0, double *ux,
                                     void *stream);
/* hpmpc_mi355x_ipm_soft_batch on the plan's soft plan with the packed default layout.  mu0 must be > 0
 * (HPMPC_MI355X_EUNSUPPORTED otherwise): the one-problem wrapper replaces mu0 <= 0 by the problem's largest cost
 * entry, a per-problem value, and the kernel takes one mu0 for the whole batch. */
int hpmpc_mi355x_ocp_soft_ipm_batch(const hpmpc_mi355x_ocp_soft_plan *plan, int nprob, int p0, int count,
                                    const double *BAbt, const double *RSQrq, const double *Z, const double *z,
                                    const double *d, double *ux, double *pi, double *lam, double *t, double *ws,
                                    int k_max, double mu0, double mu_tol, double alpha_min, int warm_start,
                                    int compute_mult, int *kk, int *ret, double *stat, void *stream);
/* The wrapper's outputs from the iterate: u, x, pi_out, lam_out and, when t_out is not null, t_out.  With a non-null
 * inf_norm_res first d_res_mpc_soft_tv over the batch into `res` (nprob * hpmpc_mi355x_ocp_soft_sizes()[19] doubles,
 * no initialisation needed; ws is not touched): per problem [r_q | r_b] 16 doubles per stage each, then r_d laid out
 * like d, then r_z laid out like Z, and after the nprob images mu per problem.  A null inf_norm_res skips the
 * residual pass and needs no res, BAbt, RSQrq, Z, z or d.  A non-null inf_norm_res on a plan with res_ok = 0 returns
 * HPMPC_MI355X_EUNSUPPORTED and launches nothing. */
int hpmpc_mi355x_ocp_soft_finish_batch(const hpmpc_mi355x_ocp_soft_plan *plan, int nprob, int p0, int count,
                                       const double *BAbt, const double *RSQrq, const double *Z, const double *z,
                                       const double *d, const double *ux, const double *pi, const double *lam,
                                       const double *t, double *res, double *u, double *x, double *pi_out,
                                       double *lam_out, double *t_out, double *inf_norm_res, void *stream);

/* ---- the KKT re-solve for device-resident batches, many right-hand sides per factor ----
 * d_kkt_solve_new_rhs_res_mpc_hard_tv (include/mpc_solvers.h:46, mpc_solvers/d_ip2_res_hard.c:1922) on a batch: the
 * last Newton system of an IPM re-solved for new b, q / r and bounds, one Riccati solve on the persisted factor per
 * right-hand-side set instead of a whole IPM solve (the feedback step of a real-time iteration, a scenario fan-out
 * over one linearisation).  Every problem takes nrhs sets; set s = p * nrhs + r belongs to problem p.  One launch,
 * one wavefront per set; the sets of a problem share its matrices and workspace, both read only.
 * Which ws is valid: the workspaces hpmpc_mi355x_ipm_batch, hpmpc_mi355x_ipm_solo or hpmpc_mi355x_ocp_ipm_batch left
 * for the same problems (same plan, same BAbt / RSQrq / DCt matrices), with at least one iteration done (kk >= 1).
 * After kk = 0 the workspace holds no factor and the result is undefined, as in the reference.  A queue solve
 * (hpmpc_mi355x_ipm_queue) reuses its per-slot workspaces and leaves no factor, so the re-solve cannot follow it.
 * The call never writes ws (nor BAbt, RSQrq, DCt, d), so any number of re-solves may follow one IPM.
 * Arrays: BAbt / RSQrq follow `lay` as in hpmpc_mi355x_ipm_batch (NULL: the packed default).  General constraints:
 * unlike the other Part-2 calls this one takes a tile plan with ng > 0 (the tile plan of an OCP plan is one), with
 * DCt problem-major in the plan's packed DCt layout (hpmpc_mi355x_ocp_offsets [17]); DCt may be null when every ng
 * is 0.  Per set, nprob * nrhs of each: d, lam, t 32 doubles per stage, ux, pi 16 doubles per stage (the layouts of
 * hpmpc_mi355x_ipm_batch); b 16 doubles per stage in state order (b_k over x_{k+1}), q 16 doubles per stage in
 * variable order [r_k | q_k].  b or q null: every set of a problem takes that vector from the augmented row of the
 * problem's BAbt_k / RSQrq_k.  scratch: nprob * nrhs * hpmpc_mi355x_kkt_scratch_doubles(plan) doubles, no
 * initialisation needed.  compute_mult = 0: pi is not solved for and returns the IPM's previous iterate.
 * Asynchronous on `stream`; synchronises with nothing (the first use of a layout uploads its stage table, as for
 * every batched call).  Only the sets of problems [p0, p0+count) are read or written; count = 0 returns 0.
 * nrhs < 1, a bad problem range, a null required pointer, a null DCt with ng > 0 or a refused launch return
 * HPMPC_MI355X_EUNSUPPORTED and write nothing. */
/* doubles of scratch per right-hand-side set */
long long hpmpc_mi355x_kkt_scratch_doubles(const hpmpc_mi355x_plan *plan);
int hpmpc_mi355x_kkt_new_rhs_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                                   int count, int nrhs, const double *BAbt, const double *RSQrq, const double *DCt,
                                   const double *b, const double *q, const double *d, double *ux, double *pi,
                                   double *lam, double *t, const double *ws, double *scratch, int compute_mult,
                                   void *stream);
/* The batched core of fortran_order_ / c_order_d_solve_kkt_new_rhs_ocp_hard_tv: the call above with nrhs = 1 and null
 * b / q on the packed default layout.  The whole wrapper is hpmpc_mi355x_ocp_pack_batch(matrices = 0) with the new
 * b, q, r and bounds, this call (ux, pi, lam, t: the OCP iterate arrays), then hpmpc_mi355x_ocp_finish_batch.
 * scratch: nprob * hpmpc_mi355x_kkt_scratch_doubles(hpmpc_mi355x_ocp_tile_plan(plan)) doubles. */
int hpmpc_mi355x_ocp_kkt_batch(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, const double *BAbt,
                               const double *RSQrq, const double *DCt, const double *d, double *ux, double *pi,
                               double *lam, double *t, const double *ws, double *scratch, void *stream);
/* The multi-set finish: the padded ux, pi, lam, t and d of nprob * nrhs re-solved sets (the arrays of
 * hpmpc_mi355x_kkt_new_rhs_batch) -> per set u, x, pi_out shaped like r, q, b and lam_out, t_out compact as
 * [lb nb | ub nb | lg ng | ug ng], all (nprob, nrhs, size) with the per-problem sizes hpmpc_mi355x_ocp_sizes reports
 * at [23..26].  The equality-box fix of hpmpc_mi355x_ocp_finish_batch is applied from the set's own d (the same loop
 * bound and comparison).  Pure data movement, one launch; t_out may be null.  The residual norms per set
 * (inf_norm_res) are out of scope: they need the set's b / q / d in a residual pass per set, which this call does
 * not run.  nrhs < 1, a bad range or a null required pointer return HPMPC_MI355X_EUNSUPPORTED and write nothing. */
int hpmpc_mi355x_ocp_unpack_sets(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, int nrhs,
                                 const double *d, const double *ux, const double *pi, const double *lam,
                                 const double *t, double *u, double *x, double *pi_out, double *lam_out,
                                 double *t_out, void *stream);

/* ---- the KKT re-solve for device-resident batches of SOFT-constrained problems, many sets per factor ----
 * The soft counterpart of hpmpc_mi355x_kkt_new_rhs_batch: after one hpmpc_mi355x_ipm_soft_batch the Newton system of a
 * linearisation re-solved for new b, q / r, bounds and linear penalties z, one Riccati solve on the factor per
 * right-hand-side set.  AN EXTENSION: the reference has no d_kkt_solve_new_rhs_* for d_ip2_mpc_soft_tv, so the call is
 * defined here.  Layouts are those of hpmpc_mi355x_ipm_soft_batch (lam, t = [lo pnb | up pnb | s0 s1 s2 s3, pns each],
 * d = [lb | ub | ls | us], Z, z = [lower | upper], idxb[k] the hard boxes then the soft ones).
 * A linearisation is a pair (Lam, tau) in the layout of lam -- Lam = lam / t at some iterate, tau that iterate's t --
 * with Zl and the Riccati factor of RSQrq_k + diag(Qx_k), both built from Lam and Z alone as the soft IPM's Hessian
 * update builds them.  For one set (b', q' = [r' | q'], d', z') the result is the affine (sigma mu = 0) Newton point
 * (ux', pi', lam', t'), the unique solution of
 *   hard box j on v = idxb[j]:        t'_lo = ux'_v - lb',  t'_up = ub' - ux'_v
 *   soft box i on v = idxb[nb + i]:   t'_0 = ux'_v - ls' + s_l,  t'_1 = us' - ux'_v + s_u,  t'_2 = s_l,  t'_3 = s_u
 *   every multiplier:                 lam' = Lam (tau - t')    (complementarity linearised with the frozen ratio Lam)
 *   slack stationarity:               Z_l s_l + z'_l - lam'_0 - lam'_2 = 0,  Z_u s_u + z'_u - lam'_1 - lam'_3 = 0
 *   stationarity in ux and the dynamics with b', in the sign conventions of d_res_mpc_soft_tv
 * so that r_q = r_b = r_d = r_z = 0 on the set's own data, with the variable of soft box i read at idxb[k][nb + i]
 * (where the IPM puts it) and its multipliers entering r_q as lam_0 - lam_1 on every stage.  No step length is taken
 * and no positivity is enforced, as in the hard re-solve.
 * refactor = 0: the linearisation a solve left.  After hpmpc_mi355x_ipm_soft_batch / hpmpc_mi355x_ocp_soft_ipm_batch
 * with kk >= 1, ws holds lam / t, 1 / t, Zl and the factor of the last iteration, all taken at iterate kk - 1; the call
 * takes Lam = lam / t and tau = 1 / (1 / t) from there and only READS ws, so any number of re-solves may follow one
 * solve.  After kk = 0 the result is undefined, as for the hard call.  lam0 and t0 are not read.
 * refactor = 1: at a given iterate.  lam0, t0 (per problem, positive on the live slots; normally the iterate the solve
 * returned) are required; a first launch, one wavefront per problem, writes 1 / t, lam / t, Qx and Zl into ws and
 * factorises, then the sets follow.  ws needs no initialisation for this, and a later refactor = 0 call reuses it.
 * Per set, nprob * nrhs of each (set s = p * nrhs + r belongs to problem p): b 16 doubles per stage in state order, q 16
 * per stage in variable order [r_k | q_k], d and z in the soft layouts (hpmpc_mi355x_soft_sizes [0], [1]); the outputs ux,
 * pi 16 per stage and lam, t in the soft layout ([2]); only live entries are written.  z null: every set takes its
 * problem's z0.  Z and z0 are per problem (Z, and one of z / z0, are required when the plan has soft boxes).  scratch:
 * nprob * nrhs * hpmpc_mi355x_soft_kkt_scratch_doubles(plan) doubles, no initialisation needed.  compute_mult = 0 skips
 * pi (not written).  BAbt / RSQrq follow `lay` as in hpmpc_mi355x_ipm_soft_batch (NULL: the packed default; shared
 * blocks allowed).  Asynchronous on `stream`; synchronises with nothing.  Only the sets of problems [p0, p0+count) are
 * read or written; count = 0 returns 0.  nrhs < 1, a bad range, a null required pointer, a refused launch or a plan with
 * no constraint on any stage (such problems have the ric_*_batch calls) return HPMPC_MI355X_EUNSUPPORTED and write
 * nothing. */
/* doubles of scratch per right-hand-side set */
long long hpmpc_mi355x_soft_kkt_scratch_doubles(const hpmpc_mi355x_soft_plan *plan);
int hpmpc_mi355x_soft_kkt_batch(const hpmpc_mi355x_soft_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                                int count, int nrhs, const double *BAbt, const double *RSQrq, const double *Z,
                                const double *z0, const double *lam0, const double *t0, const double *b,
                                const double *q, const double *d, const double *z, double *ux, double *pi, double *lam,
                                double *t, double *ws, double *scratch, int refactor, int compute_mult, void *stream);
/* The same on the dense vectors of the soft OCP front end, on the packed default layout (BAbt, RSQrq, Z, z0: the packed
 * arrays of hpmpc_mi355x_ocp_soft_pack_batch; lam0, t0: the packed iterate; ws: the solve's).  b, q, r, lb, ub and
 * optionally z are (nprob, nrhs, size) with the sizes hpmpc_mi355x_ocp_soft_sizes reports at [2], [6], [7], [8], [9],
 * [11]; a null z gives every set its problem's z0.  Three launches: a vector pack per set (the placement of
 * hpmpc_mi355x_ocp_soft_pack_batch), the call above with compute_mult = 1, and an unpack per set into u, x, pi_out,
 * lam_out, t_out (t_out may be null), all (nprob, nrhs, size) with the sizes at [20..23], lam / t compact as
 * [lo nb | up nb | 4 soft blocks of ns].  work: nprob * nrhs * hpmpc_mi355x_soft_kkt_ocp_work_doubles(plan) doubles for
 * the packed per-set vectors, scratch: nprob * nrhs * hpmpc_mi355x_soft_kkt_scratch_doubles(the plan's soft plan); neither
 * needs initialisation.  No residual norms per set.  Refusals as above, every check before the first launch. */
long long hpmpc_mi355x_soft_kkt_ocp_work_doubles(const hpmpc_mi355x_ocp_soft_plan *plan);
int hpmpc_mi355x_soft_kkt_ocp_batch(const hpmpc_mi355x_ocp_soft_plan *plan, int nprob, int p0, int count, int nrhs,
                                    const double *BAbt, const double *RSQrq, const double *Z, const double *z0,
                                    const double *lam0, const double *t0, const double *b, const double *q,
                                    const double *r, const double *lb, const double *ub, const double *z, double *u,
                                    double *x, double *pi_out, double *lam_out, double *t_out, double *ws, double *work,
                                    double *scratch, int refactor, void *stream);

/* ---- the KKT tangent solve: forward sensitivities of the re-solve, one set per parameter direction ----
 * The re-solve above is an affine map of (b, q, d): the factor is fixed, the step length is 1 and there is no line
 * search.  This call computes its linear part T directly,
 *   T(db, dq, dd) = kkt(b + db, q + dq, d + dd) - kkt(b, q, d)   in exact arithmetic, for any base (b, q, d),
 * with no base solve and no subtraction: one Riccati solve on the persisted factor per direction, without the
 * re-solve's residual pass and backup copies.  Result: (dux, dpi, dlam, dt), the directional derivative of the
 * re-solved (ux, pi, lam, t) -- e.g. d u_0 / d x_0 for a problem whose x_0 is folded into b_0 and r_0 (the feedback
 * gain of a sensitivity-based or advanced-step MPC update), or the sensitivity of the plan to a bound.  It is exactly
 * linear: the zero direction gives zeros and a direction scaled by a power of two gives the scaled result bit for bit.
 * Every problem takes ndir direction sets; set s = p * ndir + r belongs to problem p.  One launch, one wavefront per
 * set.  Layouts and conventions are the re-solve's: db 16 doubles per stage in state order, dq 16 doubles per stage
 * in variable order [dr_k | dq_k], dd 32 doubles per stage as [dlb | dub | dlg | dug], nprob * ndir sets of each; the
 * results likewise (dux, dpi 16, dlam, dt 32 doubles per stage; every element of the sets in range is written,
 * padding as zeros).  Any of db, dq, dd may be null: a zero direction (all three null give zero results).
 * Which ws is valid: exactly what is valid for hpmpc_mi355x_kkt_new_rhs_batch (an IPM of the same problems with
 * kk >= 1; not a queue solve).  Of it the call reads the factor, t^-1 and the multiplier backup; it never writes ws
 * (nor BAbt, RSQrq, DCt, the directions), so tangents and re-solves may follow one IPM in any number and order.
 * Takes tile plans with ng > 0 and layouts like the re-solve.  scratch: nprob * ndir *
 * hpmpc_mi355x_kkt_scratch_doubles(plan) doubles, no initialisation needed and no result depends on its contents.
 * compute_mult = 0: dpi is returned as zeros.  Asynchronous on `stream`, synchronises with nothing; only the sets of
 * problems [p0, p0+count) are read or written; count = 0 returns 0.  ndir < 1, a bad range, a null required pointer,
 * a null DCt with ng > 0 or a refused launch return HPMPC_MI355X_EUNSUPPORTED and write nothing.
 * Reverse mode is the adjoint solve below, and the gradients with respect to the matrices follow it
 * (hpmpc_mi355x_ocp_matrix_grads_batch).  Directions in the matrices (A, B, Q, S, R, C, D) are a seed launch in front
 * of this solve: hpmpc_mi355x_ocp_matrix_dirs_batch / hpmpc_mi355x_ocp_tangent_data_batch at the end of this header.
 * Out of scope, absent rather than half-built: per-set residual norms. */
int hpmpc_mi355x_kkt_tangent_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                                   int count, int ndir, const double *BAbt, const double *RSQrq, const double *DCt,
                                   const double *db, const double *dq, const double *dd, double *dux, double *dpi,
                                   double *dlam, double *dt, const double *ws, double *scratch, int compute_mult,
                                   void *stream);
/* The same for dense directions and dense results on an OCP plan (packed default layout).  dirs: only the vector
 * entries b, q, r, lb, ub, lg, ug are read; stride[i] is the number of doubles between consecutive SETS (nprob * ndir
 * of them, problem-major), a null pointer is a zero direction, and a non-null matrix entry (A, B, Q, S, R, C, D) is
 * refused with HPMPC_MI355X_EUNSUPPORTED (hpmpc_mi355x_ocp_tangent_data_batch takes them).  Results per set: du shaped like r, dx like q, dpi like b, dlam / dt compact
 * as [lb nb | ub nb | lg ng | ug ng]; all (nprob, ndir, size) with the per-problem sizes of hpmpc_mi355x_ocp_sizes
 * [23..26].  The equality-box fix of hpmpc_mi355x_ocp_finish_batch is NOT applied to tangents: the fix overwrites
 * u with the bound where lb == ub, a property of the base point; the tangent of such an input is what the Newton
 * system gives (zero up to the rounding of 1 / t), not the bound's direction.  Seeding and unpacking are the
 * prologue and epilogue of the one kernel launch: no host copy, no synchronisation, no padded array of the caller's.
 * scratch as above. */
int hpmpc_mi355x_ocp_tangent_batch(const hpmpc_mi355x_ocp_plan *plan, const hpmpc_mi355x_ocp_data *dirs, int nprob,
                                   int p0, int count, int ndir, const double *BAbt, const double *RSQrq,
                                   const double *DCt, double *du, double *dx, double *dpi, double *dlam, double *dt,
                                   const double *ws, double *scratch, int compute_mult, void *stream);

/* ---- the KKT adjoint solve: reverse-mode sensitivities of the re-solve, one set per scalar loss ----
 * The transpose of the tangent map T above.  For cotangents (gux, gpi, glam, gt) of the re-solved (ux, pi, lam, t) --
 * the gradient of a scalar loss with respect to the iterate -- the call returns (bbar, qbar, dbar) = T' g, that loss's
 * gradient with respect to every element of b, q / r and the bounds d, in ONE Riccati solve on the persisted factor
 * where forward mode takes one per parameter direction; e.g. d u_0 / d x_0 from nu[0] sets (cotangent e_i on u_0)
 * instead of nx0 tangent sets.  With w = lam * t^-1 on every [lb | ub | lg | ug] slot and C the constraint rows:
 *   h = gt - w glam,  c_j = h_lo - h_up;   (y_ux, y_pi) = S(gux + C' c, gpi), S the tangent's Riccati solve;
 *   qbar = y_ux,  bbar = y_pi,  z = C y_ux,  dbar_lo = -h_lo - w_lo z,  dbar_up = h_up - w_up z.
 * S is minus the inverse of the symmetric KKT matrix, so this is T' exactly in exact arithmetic.  Where the
 * reference's x-pivot clamp fired on a stage, the persisted factor is not that of a symmetric system and the call is
 * DEFINED as the three steps above, not as an exact transpose.  It is exactly linear: zero cotangents give zeros and
 * cotangents scaled by a power of two give the scaled result bit for bit.
 * Every problem takes nadj cotangent sets; set s = p * nadj + r belongs to problem p.  One launch, one wavefront per
 * set.  Layouts are the tangent's: gux / qbar 16 doubles per stage in variable order, gpi / bbar 16 in state order,
 * glam / gt / dbar 32 as [lb | ub | lg | ug], nprob * nadj sets of each.  Any cotangent may be null: zero.  qbar and
 * dbar are required; every element of them (and of bbar) in the sets in range is written, padding as zeros.  A null
 * bbar skips the multiplier half of the solve and nothing of b's is written.
 * Which ws is valid: exactly what is valid for hpmpc_mi355x_kkt_new_rhs_batch (an IPM of the same problems with
 * kk >= 1; not a queue solve).  Of it the call reads the factor, t^-1 and the multiplier backup; it never writes ws
 * (nor BAbt, RSQrq, DCt, the cotangents), so adjoints, tangents and re-solves may follow one IPM in any number and
 * order.  Takes tile plans with ng > 0 and layouts like the re-solve.  scratch: nprob * nadj *
 * hpmpc_mi355x_kkt_scratch_doubles(plan) doubles, no initialisation needed and no result depends on its contents.
 * Asynchronous on `stream`, synchronises with nothing; only the sets of problems [p0, p0+count) are read or written;
 * count = 0 returns 0.  nadj < 1, a bad range, a null required pointer, a null DCt with ng > 0 or a refused launch
 * return HPMPC_MI355X_EUNSUPPORTED and write nothing.
 * Gradients with respect to the matrices (A, B, Q, S, R, C, D) are outer products of this adjoint solution with the
 * base iterate: hpmpc_mi355x_ocp_matrix_grads_batch / hpmpc_mi355x_ocp_adjoint_data_batch below; the Python package
 * wraps them in a torch.autograd.Function (hpmpc_amd.ocp_autograd).  Out of scope, absent rather than half-built: an
 * adjoint of the IPM iteration itself; soft-constraint and wide-stage plans. */
int hpmpc_mi355x_kkt_adjoint_batch(const hpmpc_mi355x_plan *plan, const hpmpc_mi355x_layout *lay, int nprob, int p0,
                                   int count, int nadj, const double *BAbt, const double *RSQrq, const double *DCt,
                                   const double *gux, const double *gpi, const double *glam, const double *gt,
                                   double *bbar, double *qbar, double *dbar, const double *ws, double *scratch,
                                   void *stream);
/* The same for dense cotangents and dense gradients on an OCP plan (packed default layout).  gu shaped like r, gx
 * like q, gpi like b, glam / gt compact as [lb nb | ub nb | lg ng | ug ng]: (nprob, nadj, size) with the per-problem
 * sizes of hpmpc_mi355x_ocp_sizes [23..26]; a null one is zero.  The gradients gb, gq, gr, glb, gub, glg, gug have the
 * shapes of the dense data arrays, (nprob, nadj, size) with the sizes at [2], [6], [7], [8], [9], [12], [13]; a null
 * one is not wanted, at least one is required, and a null gb skips the multiplier half of the solve.  The placements
 * are the exact transposes of the dense tangent call's (the equality-box fix is not part of either), and they are
 * the prologue and epilogue of the one kernel launch.  scratch as above. */
int hpmpc_mi355x_ocp_adjoint_batch(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, int nadj,
                                   const double *BAbt, const double *RSQrq, const double *DCt, const double *gu,
                                   const double *gx, const double *gpi, const double *glam, const double *gt,
                                   double *gb, double *gq, double *gr, double *glb, double *gub, double *glg,
                                   double *gug, const double *ws, double *scratch, void *stream);

/* ---- gradients with respect to the matrices A, B, Q, S, R, C, D, from the adjoint solution ----
 * The residuals of the KKT system (d_res_res_mpc_hard_tv) carry b, q / r and d with unit coefficients and are bilinear
 * in (matrices, iterate).  At a fixed base iterate z = (ux, pi, lam), with ux_k = [u_k | x_k], a perturbation of the
 * matrices moves them by
 *   dr_b[k] = dA_k x_k + dB_k u_k,   dr_q[k] = dRSQ_k ux_k + dBAbt_k pi_k + dDCt_k (lam_ug,k - lam_lg,k),
 *   dr_d[k] = -(dC_k x_k + dD_k u_k)  on both the lg and the ug slots.
 * The MATRIX TANGENT is defined as T_M(dtheta) = T(dr_b, dr_q, dr_d) with T the tangent map above, and these calls
 * return its transpose: with (bbar, qbar = [rbar | qxbar], dbar) = T' g the adjoint solution of a cotangent set, per
 * stage k, in the dense shapes of hpmpc_mi355x_ocp_data,
 *   gA_k = bbar_k x_k' + pi_k qxbar_k'                 gB_k = bbar_k u_k' + pi_k rbar_k'
 *   gQ_k = (qxbar_k x_k' + x_k qxbar_k') / 2           gR_k = (rbar_k u_k' + u_k rbar_k') / 2
 *   gS_k = rbar_k x_k' + u_k qxbar_k'
 *   gC_k = w_k qxbar_k' - s_k x_k'                     gD_k = w_k rbar_k' - s_k u_k'
 * with w_k = lam_ug,k - lam_lg,k and s_k = dbar_lg,k + dbar_ug,k.  Conventions: pi_k is the multiplier of stage k's
 * dynamics x_{k+1} = A_k x_k + B_k u_k + b_k and has nx[k+1] entries; gQ and gR are the gradients for SYMMETRIC
 * perturbations -- <gQ, dQ> is the directional derivative for dQ = dQ', the kernels read only the lower triangle of
 * RSQrq -- and are symmetric bit for bit; S is an ordinary nu x nx block.  Blocks of a time-invariant matrix are not
 * summed over the stages: the caller sums them.
 * What the quantity is: the exact transpose of T_M, the linearised KKT system on the persisted factor.  It is NOT the
 * derivative of a fully converged solve: the factor belongs to the last Newton system of the IPM, which was formed one
 * iterate before the returned point.  Finite differences of whole IPM solves (mu_tol 1e-10) agree with <G, dtheta> to
 * between 4e-5 and 2e-3 relative on the test problems.  The vector gradients of the adjoint call rest on the same
 * factor.  Exactly linear in the cotangent like the adjoint solve.
 * grads: ptr[i] null: gradient i is not wanted; stride[i]: doubles between consecutive SETS (nprob * nadj of them,
 * problem-major), at least the array's per-problem size.  Every element of a wanted array of the sets in range is
 * written, nothing else; no atomics, no initialisation needed. */
typedef struct {
    double *ptr[HPMPC_MI355X_OCP_NARRAYS];       /* device pointers; null: not wanted */
    long long stride[HPMPC_MI355X_OCP_NARRAYS];  /* doubles between SETS */
} hpmpc_mi355x_ocp_grads;
/* The core: one launch (hk_ocp_matgrad), one workgroup per (stage, set), from padded arrays.  ux, pi, lam: the base
 * iterate per problem in the solver's padded layouts (16, 16, 32 doubles per stage) -- the IPM's, or a re-solve's.
 * bbar, qbar, dbar: the outputs of hpmpc_mi355x_kkt_adjoint_batch, nprob * nadj sets.  ux and qbar are required; pi and
 * bbar when gA or gB is wanted; lam and dbar when the plan has ng > 0 and gC or gD is wanted.  A non-null vector entry
 * of grads (b, q, r, lb, ub, lg, ug) is refused.  Asynchronous on `stream`; only the sets of problems [p0, p0+count)
 * are read or written; count = 0 returns 0.  nadj < 1, a bad range, a null plan, a null required pointer, no wanted entry,
 * a stride below the array's size or a refused launch return HPMPC_MI355X_EUNSUPPORTED and write nothing. */
int hpmpc_mi355x_ocp_matrix_grads_batch(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, int nadj,
                                        const double *ux, const double *pi, const double *lam, const double *bbar,
                                        const double *qbar, const double *dbar, const hpmpc_mi355x_ocp_grads *grads,
                                        void *stream);
/* Gradients with respect to any of the fourteen data arrays in one call: the launch of hpmpc_mi355x_ocp_adjoint_batch
 * (dense cotangents gu, gx, gpi, glam, gt as there; the vector entries of grads are its gb, gq, gr, glb, gub, glg, gug
 * and come out bit for bit the same), then the core launch above on the same stream, reading qbar, bbar and dbar from
 * each set's scratch block: no padded array of the caller's, no host synchronisation.  ux, pi, lam: the base iterate
 * as above, required as above when a matrix entry is wanted.  Wanting gA or gB forces the multiplier half of the solve
 * even when gb is null.  ws and scratch as for the adjoint call.  Refusals as above and as the adjoint call's. */
int hpmpc_mi355x_ocp_adjoint_data_batch(const hpmpc_mi355x_ocp_plan *plan, int nprob, int p0, int count, int nadj,
                                        const double *BAbt, const double *RSQrq, const double *DCt, const double *ux,
                                        const double *pi, const double *lam, const double *gu, const double *gx,
                                        const double *gpi, const double *glam, const double *gt,
                                        const hpmpc_mi355x_ocp_grads *grads, const double *ws, double *scratch,
                                        void *stream);

/* ---- directions in all fourteen data arrays: the matrix tangent T_M, forward ----
 * The forward evaluation of the map whose transpose the matrix gradients above are.  At a fixed base iterate z = (ux, pi,
 * lam), ux_k = [u_k | x_k], a direction dtheta in the data moves the residuals of the KKT system by the SEED ROW, per
 * stage k,
 *   db_k    = db + dA_k x_k + dB_k u_k
 *   dr_k    = dr + sym(dR_k) u_k + dS_k x_k + dB_k' pi_k + dD_k' w_k
 *   dq_k    = dq + sym(dQ_k) x_k + dS_k' u_k + dA_k' pi_k + dC_k' w_k
 *   dd_lg,k = dlg - (dC_k x_k + dD_k u_k),   dd_ug,k = dug - (dC_k x_k + dD_k u_k),   dd_lb = dlb,   dd_ub = dub
 * with w_k = lam_ug,k - lam_lg,k, and the tangent is T_M(dtheta) = T(db, [dr | dq], dd) with T the tangent map of
 * hpmpc_mi355x_kkt_tangent_batch.  Conventions: pi_k is the multiplier of stage k's dynamics and has nx[k+1] entries;
 * stage N has no A, B, R, S, D block; sym(M) = (M + M') / 2, so dQ and dR need not be symmetric -- only their
 * symmetric parts act, as the kernels read only the lower triangle of RSQrq -- and <gQ, dQ>, <gR, dR> pair exactly with
 * the symmetric-perturbation gradients of hpmpc_mi355x_ocp_matrix_grads_batch for ANY dQ, dR: <g, T_M(dtheta)> =
 * <G, dtheta> over all fourteen arrays, up to rounding.  Blocks of a time-invariant matrix are separate entries: the
 * caller repeats its direction over the stages.
 * What the quantity is: the linearised KKT system on the persisted factor, the exact forward twin of the matrix
 * gradients.  It is NOT the derivative of a fully converged solve: the factor belongs to the last Newton system of the
 * IPM, which was formed one iterate before the returned point (the figures of the matrix gradients' paragraph apply).
 * Exactly linear in the direction: directions scaled by a power of two give the scaled result bit for bit.
 * dirs: an hpmpc_mi355x_ocp_data whose stride[i] counts the doubles between consecutive SETS (nprob * ndir of them,
 * problem-major), at least the array's per-problem size.  All fourteen entries are read and any may be null: a null
 * vector entry is a zero direction, a null matrix entry contributes no term (not an added zero, so with every matrix
 * entry null the row is the vector directions' bit for bit).  Each element's terms are summed in one fixed order: the
 * vector direction first, then the products in the order of the formulas above from left to right, within a matrix by
 * rising index; a set's row does not depend on the other sets of the call. */
/* The core: one launch (hk_ocp_matdir), one workgroup per (stage, set).  ux, pi, lam: the base iterate per problem in
 * the solver's padded layouts (16, 16, 32 doubles per stage) -- the IPM's, or a re-solve's.  db, dq, dd: the seed rows,
 * padded per-set arrays (16 / 16 / 32 doubles per stage, nprob * ndir sets), directly usable as the db, dq, dd of
 * hpmpc_mi355x_kkt_tangent_batch; every element of the sets in range is written, padding as zeros, nothing else is,
 * and no input is written.  ux is required; pi when an A or B direction is given; lam when the plan has ng > 0 and a
 * C or D direction is given.  Asynchronous on `stream`; only the sets of problems [p0, p0+count) are read or written;
 * count = 0 returns 0.  ndir < 1, a bad range, a null plan, a null required pointer, a stride below the array's
 * per-problem size for a given entry or a refused launch return HPMPC_MI355X_EUNSUPPORTED and write nothing. */
int hpmpc_mi355x_ocp_matrix_dirs_batch(const hpmpc_mi355x_ocp_plan *plan, const hpmpc_mi355x_ocp_data *dirs, int nprob,
                                       int p0, int count, int ndir, const double *ux, const double *pi,
                                       const double *lam, double *db, double *dq, double *dd, void *stream);
/* The tangent for directions in any of the fourteen arrays in one call: the seed launch above into each set's scratch
 * block, then the launch of hpmpc_mi355x_ocp_tangent_batch on the same stream with its seeding skipped and its
 * unpacking unchanged: no padded array of the caller's, no host synchronisation.  Results du, dx, dpi, dlam, dt, and
 * BAbt, RSQrq, DCt, ws, scratch (hpmpc_mi355x_kkt_scratch_doubles per set) and compute_mult as for that call; ux, pi,
 * lam as above.  With every matrix entry null the results are bit for bit those of hpmpc_mi355x_ocp_tangent_batch.
 * Every check of both launches comes before the first; refusals as above and as the tangent call's. */
int hpmpc_mi355x_ocp_tangent_data_batch(const hpmpc_mi355x_ocp_plan *plan, const hpmpc_mi355x_ocp_data *dirs, int nprob,
                                        int p0, int count, int ndir, const double *BAbt, const double *RSQrq,
                                        const double *DCt, const double *ux, const double *pi, const double *lam,
                                        double *du, double *dx, double *dpi, double *dlam, double *dt, const double *ws,
                                        double *scratch, int compute_mult, void *stream);

#ifdef __cplusplus
}
#endif
#endif /* HPMPC_MI355X_H_ */

"""Shared by tests/test_ocp_soft_host.py and tests/test_gpu_ocp_soft.py: the inputs of the soft OCP front end's tests
(hpmpc_mi355x_ocp_soft_*, hpmpc_amd/ocp_soft.py) in the interface form of oracle/iface_oracle.py, the admitted seeds
with the oracle's iteration counts, and the expected packed arrays.

Shapes:
  D   IO.random_soft_iface_problem(5, 4, 2): the reference driver's shape (hard input boxes, soft state boxes); res_ok
  Q   N = 3 with nb > nu on an inner stage (stage 1: nu 2, nb 4), so the reference's soft residual, which reads
      idxb[k][nu + i], and a reading at idxb[k][nb + i] name different variables; res_ok
  G*  the shapes of the two fixed-mu0 iface_soft goldens: the neighbours of a golden inside its batch
  C   the draws of tests/soft_cases.py through soft_iface_from_qp, with z given (admitted by that module: the SoftQP
      the front end packs is the draw itself, bit for bit, tests/test_ocp_soft_host.py)

Admission rule for D, Q and G* (the ADMIT rule of tests/soft_cases.py; tests/test_ocp_soft_host.py checks it): a
(shape, seed) pair is used only if oracle/liboracle.so and oracle/liboracle_fma.so return identical kk and ret on
IO.to_soft_qp(P) (z = 0, as the front end packs a null z), the two differ by at most 25 % of every TOL_SOFT gate,
and the run converges (ret 0).  No test takes a divergence escape.
"""
import os
import sys

import numpy as np

import soft_cases as SC
from hpmpc_amd.ocp import rup
from hpmpc_amd.ocp_soft import soft_iface_from_qp
from hpmpc_amd.soft import pack_soft_batch, random_soft_qp

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import iface_oracle as IO  # noqa: E402

ARGS = dict(SC.ARGS)  # k_max 50, mu0 100, mu_tol 1e-6, alpha_min 1e-8
# (nx[2] = 7, not 6: with nx = 6 the reference reads b_1 outside BAbt_1 and the soft plan refuses the shape)
Q_SHAPE = dict(N=3, nx=[0, 5, 7, 4], nu=[2, 2, 1, 0], nb=[2, 4, 1, 2], ns=[0, 3, 4, 2])
# golden name -> (N, nx, nu), the golden's seed, its mu0 (tests/golden/make_golden.py iface_soft)
GOLDENS = {"iface_soft_N12_nx8_nu3": ((12, 8, 3), 12, 100.0), "iface_soft_N8_nx12_nu4": ((8, 12, 4), 8, 50.0)}

# shape -> the admitted draws (seed, kk, ret, spread): kk / ret are the oracle's (identical in its FMA build), spread
# the worst distance of the two oracle builds as a share of its TOL_SOFT gate, measured when the seed was admitted.
# The goldens' own seeds (12, 8) are held to the reference build by their golden files; here they are admitted on
# the oracle builds like their neighbours.
DRAWS = {
    "D": [(0, 9, 0, 1.5e-5), (1, 9, 0, 4.8e-4), (2, 10, 0, 6.8e-3), (3, 11, 0, 3.1e-2)],
    # with z = 0 and x0_scale 2 most draws of Q end at alpha_min (ret 2): of seeds 0 .. 13 these three converge
    "Q": [(3, 10, 0, 6.4e-3), (7, 9, 0, 2.5e-3), (13, 10, 0, 8.3e-2)],
    "iface_soft_N12_nx8_nu3": [(1, 10, 0, 2.5e-3), (12, 10, 0, 1.9e-2), (2, 11, 0, 1.5e-2)],  # the golden in the middle
    "iface_soft_N8_nx12_nu4": [(1, 9, 0, 7.7e-4), (8, 11, 0, 4.5e-2), (3, 11, 0, 1.8e-2)],
}
GOLDEN_AT = 1  # the golden's place in its batch
C_SHAPES = ("odd", "full16", "N1", "softonly", "x0_u")


def args_of(shape):
    return dict(ARGS, mu0=GOLDENS[shape][2]) if shape in GOLDENS else dict(ARGS)


def make(shape, seed):
    """The interface-form problem of a (shape, seed) pair.  D, Q, G*: the front end gets no z (P["z"] is what the
    reference wrapper would be handed and ignore); C shapes: z is given."""
    if shape == "D":
        return IO.random_soft_iface_problem(5, 4, 2, seed=seed)
    if shape == "Q":
        return soft_iface_from_qp(random_soft_qp(**Q_SHAPE, seed=seed))
    if shape in GOLDENS:
        return IO.random_soft_iface_problem(*GOLDENS[shape][0], seed=seed)
    return soft_iface_from_qp(SC.make(shape, seed))


def seeds(shape):
    return SC.seeds(shape) if shape in SC.CASES else [d[0] for d in DRAWS[shape]]


def kks(shape):
    return SC.kks(shape) if shape in SC.CASES else [d[1] for d in DRAWS[shape]]


def problems(shape):
    return [make(shape, s) for s in seeds(shape)]


def soft_qp(P, with_z):
    """The SoftQP the front end packs: IO.to_soft_qp, with z filled like Z when the front end is given z."""
    sq = IO.to_soft_qp(P)
    if with_z:
        for k in range(P["N"] + 1):
            ns, pns = P["ns"][k], rup(P["ns"][k], 4)
            sq.z[k][:ns] = P["z"][k][:ns]
            sq.z[k][pns:pns + ns] = P["z"][k][ns:2 * ns]
    return sq


def expected_packed(Ps, with_z):
    """BAbt, RSQrq, d, Z, z (nprob, size) as pack_soft_batch lays out the SoftQPs of ``Ps``."""
    pk = pack_soft_batch([soft_qp(P, with_z) for P in Ps])
    return {k: pk[k] for k in ("BAbt", "RSQrq", "d", "Z", "z")}


def soft_rd_max(P, ux, t, reading):
    """max |r_d| of d_res_mpc_soft_tv over the elements the wrapper visits, restated in numpy with the variable of soft
    constraint i of stage k read at idxb[k][nu_k + i] (reading "nu": the reference, d_res_ip_soft.c:107) or at
    idxb[k][nb_k + i] (reading "nb": where the IPM puts it).  ux / t: per-stage lists in the solver's padded layouts."""
    m = 0.0
    for k in range(P["N"] + 1):
        nu, nb, ns = P["nu"][k], P["nb"][k], P["ns"][k]
        pnb, pns = rup(nb, 4), rup(ns, 4)
        ib, os_ = P["hidxb"][k], 2 * pnb
        lb, ub, tk, x = P["lb"][k], P["ub"][k], np.asarray(t[k]), np.asarray(ux[k])
        for j in range(nb):
            m = max(m, abs(x[ib[j]] - lb[j] - tk[j]), abs(-x[ib[j]] + ub[j] - tk[pnb + j]))
        for j in range(ns):
            xv = x[ib[(nu if reading == "nu" else nb) + j]]
            m = max(m, abs(tk[os_ + 2 * pns + j] + xv - lb[nb + j] - tk[os_ + j]),
                    abs(tk[os_ + 3 * pns + j] - xv + ub[nb + j] - tk[os_ + pns + j]))
    return m

"""The admission rule of tests/soft_kkt_cases.py (no GPU): what qualifies the numpy reference the GPU tests of the soft
KKT re-solve (tests/test_gpu_soft_kkt.py) are held to.

For every (case, draw, set) the un-eliminated system (newton_reference) and the slack-eliminated one
(newton_eliminated) agree within 25 % of each TOL_SOFT gate, and the residuals of the reference solution on the set's own
data vanish within 1e-9 max(1, largest |entry| of the set's vectors): on the shapes where idxb[k][nu + i] and
idxb[k][nb + i] coincide through the oracle's d_res_mpc_soft_tv, which pins the signs (pi's among them), on every shape
through the numpy restatement with the "nb" reading.

The reference's residual takes the multipliers of a soft box into r_q as lam_0 - lam_1 on stages k < N but as
-lam_2 + lam_3 on stage N (d_res_ip_soft.c:220; oracle/hpmpc_oracle_soft.c restates it).  With r_z = 0 the two differ by
(Z_l s_l + z_l) - (Z_u s_u + z_u) on the rows of stage N that carry a soft box, so there the oracle's r_q is compared
after that known difference is taken out; every other row and r_b, r_d, r_z are held as they come.

Measured when the rule was last evaluated (seeds 0 .. 9, three sets each): every draw of every case is admitted; the
worst formulation spread is 5.7e-7 of its gate (iface_soft_N12_nx8_nu3 seed 8) and the worst residual 4.6e-6 of its
bound.  Each case keeps its first six draws.
"""
import numpy as np
import pytest

import ocp_soft_cases as OC
import soft_kkt_cases as K


@pytest.mark.parametrize("case", K.CASES)
def test_admission(case):
    got = []
    for seed in K.SEEDS:
        ok, fig = K.admit(case, seed)
        print(f"{case} seed {seed}: spread {fig['share']:.2e} of the gate, residual {fig['res']:.2e} of the bound, "
              f"{'admitted' if ok else 'refused'}")
        if ok and len(got) < K.MAX_DRAWS:
            got.append(seed)
    assert len(got) >= K.MIN_DRAWS, (case, got)
    assert got == K.admitted(case), (case, got)


def _stage_N_quirk(P, S, ref):
    """What the reference's stage-N r_q adds on the rows of soft boxes: -lam_2 + lam_3 in place of lam_0 - lam_1."""
    N = P["N"]
    _, nx, nb, ns, pnb, pns = K.sizes(P, N)
    lam, o, ib = ref["lam"][N], 2 * pnb, np.asarray(P["hidxb"][N])
    corr = np.zeros(nx)
    for i in range(ns):
        corr[ib[nb + i]] += (lam[o + i] - lam[o + pns + i]) - (-lam[o + 2 * pns + i] + lam[o + 3 * pns + i])
    return corr


@pytest.mark.parametrize("case", K.ORACLE_RES)
def test_reference_solution_has_no_oracle_residual(oracle, case):
    for seed in K.admitted(case):
        P, lam, t, sets = K.draw(case, seed)
        assert all(P["nu"][k] == P["nb"][k] for k in range(P["N"]) if P["ns"][k] > 0), "nu and nb readings coincide"
        Lam = [l / tt for l, tt in zip(lam, t)]
        for r, S in enumerate(sets):
            ref = K.newton_reference(P, Lam, t, S)
            sq = OC.soft_qp(K.with_set(P, S), True)
            pad = lambda v, n: np.r_[np.asarray(v, dtype=np.float64), np.zeros(n)]
            q = [pad(K._grad(P, S, k), 8) for k in range(P["N"] + 1)]
            res = oracle.residuals_soft(sq, q, [pad(v, 8) for v in ref["ux"]], [pad(v, 8) for v in ref["pi"]],
                                        [pad(v, 8) for v in ref["lam"]], [pad(v, 8) for v in ref["t"]])
            # the sign of the difference follows the oracle's final negation of r_q
            res["rq"][P["N"]][:P["nx"][P["N"]]] -= _stage_N_quirk(P, S, ref)
            bound = K.RES_TOL * K.set_scale(S)
            for key, n in (("rq", lambda k: sq.nux(k)), ("rb", lambda k: int(sq.nx[k + 1])),
                           ("rd", lambda k: len(res["rd"][k])), ("rz", lambda k: len(res["rz"][k]))):
                m = max(float(np.max(np.abs(np.asarray(v)[:n(k)]), initial=0.0)) for k, v in enumerate(res[key]))
                print(f"{case} seed {seed} set {r}: max |{key}| {m:.2e} (bound {bound:.1e})")
                assert m <= bound, (case, seed, r, key, m)

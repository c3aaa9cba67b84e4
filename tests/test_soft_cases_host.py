"""The soft-constraint IPM's random-structure cases (tests/soft_cases.py) on the CPU: the generator's invariants, the
admission rule on the pinned (case, seed) pairs, and the restated landing places of the reference's stray
soft-gradient write.  The oracle is held to the reference on these shapes by the soft_rs_* goldens
(tests/test_oracle_golden.py)."""
import os

import numpy as np
import pytest

import soft_cases as SC
from hpmpc_amd.ocp import rup, unpack_lib4
from hpmpc_amd.soft import random_soft_qp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = list(SC.CASES)


@pytest.fixture(scope="module")
def oracle_fma(oracle):  # after `oracle`: that fixture builds both libraries where they are missing
    from hpmpc_amd.cabi import HpmpcAPI, load

    return HpmpcAPI(load(os.path.join(ROOT, "oracle", "liboracle_fma.so")), "orc_")


@pytest.mark.parametrize("name", NAMES)
def test_generator_invariants(name):
    c = SC.CASES[name]
    a, b = SC.make(name, 11), SC.make(name, 12)
    other = SC.make(name, 11, structure_seed=1)
    N = c["N"]
    assert a.N == N and int(a.nu[N]) == 0
    scattered = differs = False
    for k in range(N + 1):
        nb, ns, nux = int(a.nb[k]), int(a.ns[k]), a.nux(k)
        assert (int(a.nx[k]), nb, ns) == (c["nx"][k], c["nb"][k], c["ns"][k])
        ib = a.idxb[k][:nb + ns]
        assert len(set(ib.tolist())) == nb + ns and (ib >= 0).all() and (ib < nux).all(), k
        assert np.array_equal(ib[:nb], np.sort(ib[:nb])) and np.array_equal(ib[nb:], np.sort(ib[nb:])), k
        assert np.array_equal(ib, b.idxb[k][:nb + ns]), k  # structure_seed alone draws idxb
        scattered |= bool((np.diff(ib) < 0).any())
        differs |= not np.array_equal(ib, other.idxb[k][:nb + ns])
        pnb, pns = rup(nb, 4), rup(ns, 4)
        d = a.d[k]
        assert d.size == 2 * pnb + 2 * pns + 4 and a.Z[k].size == a.z[k].size == 2 * pns + 4
        live = np.r_[0:nb, pnb:pnb + nb, 2 * pnb:2 * pnb + ns, 2 * pnb + pns:2 * pnb + pns + ns].astype(int)
        pad = np.setdiff1d(np.arange(d.size), live)
        assert (d[pad] == 0).all() and (d[live] != 0).all(), k
        assert (d[:nb] < 0).all() and (d[pnb:pnb + nb] > 0).all(), k
        lz = np.r_[0:ns, pns:pns + ns].astype(int)
        pz = np.setdiff1d(np.arange(2 * pns + 4), lz)
        for v in (a.Z[k], a.z[k]):
            assert (v[pz] == 0).all() and (v[lz] > 0).all(), k
            assert ns == 0 or len(set(v[lz].tolist())) == 2 * ns, k  # drawn per element
        M = unpack_lib4(a.RSQrq[k], nux + 1, nux)
        H = M[:nux]
        assert np.allclose(H, H.T) and (np.linalg.eigvalsh(H) >= 1.0 - 1e-12).all(), k
        if int(a.nu[k]) and int(a.nx[k]):
            assert np.abs(H[int(a.nu[k]):, :int(a.nu[k])]).min() > 0, k  # a non-zero S block
        assert not np.array_equal(a.RSQrq[k], b.RSQrq[k]), k  # the data follow `seed`
    if name not in ("N1", "softonly"):  # softonly has one sorted part per stage
        assert scattered  # some stage's idxb is not ascending
    assert differs
    again = SC.make(name, 11)
    for f in ("BAbt", "RSQrq", "d", "Z", "z"):
        assert all(np.array_equal(x, y) for x, y in zip(getattr(a, f), getattr(again, f))), f


def test_generator_covers_what_the_mass_spring_shape_fixes():
    sq = SC.make("soft_u", 0)
    k_in = [k for k in range(sq.N) if (sq.idxb[k][int(sq.nb[k]):int(sq.nb[k] + sq.ns[k])] < int(sq.nu[k])).any()]
    assert k_in  # soft boxes on inputs
    assert any(int(sq.nb[k]) == 0 and int(sq.ns[k]) > 0 for k in range(1, sq.N))  # inner stage, soft boxes only
    assert all(int(SC.make(n, 0).nx[0]) > 0 for n in ("x0_u", "x0_box"))  # a variable x_0
    odd = SC.make("odd", 0)
    assert {3, 7, 11} <= set(odd.nx.tolist())
    assert any(int(odd.ns[k]) % 4 and rup(int(odd.nb[k]), 4) != int(odd.nb[k]) for k in range(odd.N + 1))
    full = SC.make("full16", 0)
    assert [int(full.nb[k] + full.ns[k]) for k in (1, 2, 3)] == [16, 16, 16]


def test_generator_asserts_the_product_limits():
    with pytest.raises(AssertionError):  # round_up(nu, 4) + nx > 16
        random_soft_qp(2, [0, 12, 12], [5, 5, 0], [1, 1, 1], [1, 1, 1], seed=0)
    with pytest.raises(AssertionError):  # more boxes than variables
        random_soft_qp(2, [0, 4, 4], [2, 2, 0], [2, 3, 2], [1, 4, 1], seed=0)
    with pytest.raises(AssertionError):  # nx = 6: the reference reads b_k outside BAbt_k (stride round_up(nx, 4))
        random_soft_qp(2, [0, 6, 6], [2, 2, 0], [1, 1, 1], [1, 1, 1], seed=0)


@pytest.mark.parametrize("name", NAMES)
def test_admission_rule_holds(oracle, oracle_fma, name):
    """Every pinned (case, seed): the two oracle builds agree on kk / ret (the pins), differ by at most ADMIT of
    every TOL_SOFT gate, and the run converges -- or, at x0_box, takes its early exit."""
    draws = SC.CASES[name]["draws"]
    assert len(draws) >= 3
    for seed, kk, ret, _ in draws:
        sq = SC.make(name, seed)
        o, f = oracle.ipm_soft(sq.copy(), **SC.ARGS), oracle_fma.ipm_soft(sq.copy(), **SC.ARGS)
        assert (o["kk"], o["ret"]) == (f["kk"], f["ret"]) == (kk, ret), (name, seed, o["kk"], o["ret"], f["kk"], f["ret"])
        share = SC.gate_share(SC.soft_errors(sq, f, o))
        print(f"{name} seed {seed}: kk {kk} ret {ret}, spread " + " ".join(f"{k} {v:.1e}" for k, v in share.items()))
        assert max(share.values()) <= SC.ADMIT, (name, seed, share)
        assert ret == 0 or (name == "x0_box" and ret == 2 and kk <= 4), (name, seed)
    if name == "odd":
        assert len(set(SC.kks(name))) > 1  # the waves of its batch retire at different iterations


def test_warm_start_of_odd_is_admitted(oracle, oracle_fma):
    sq = SC.make("odd", SC.seeds("odd")[0])
    kw = dict(SC.ARGS, warm_start=1, ux=SC.warm_ux(sq))
    o, f = oracle.ipm_soft(sq.copy(), **kw), oracle_fma.ipm_soft(sq.copy(), **kw)
    assert (o["kk"], o["ret"]) == (f["kk"], f["ret"]) == (SC.WARM_KK, 0)
    assert max(SC.gate_share(SC.soft_errors(sq, f, o)).values()) <= SC.ADMIT


def test_stray_targets_at_stray():
    sq = SC.make("stray", 0)
    hits, refused = SC.soft_stray_targets(sq)
    assert not refused
    assert len(hits) == sum(int(sq.ns[k]) for k in range(sq.N + 1) if sq.nb[k] > 0)
    later = [h for h in hits if h["array"] == "qx" and h["live"] and h["j"] > h["k"] and h["j"] // 4 == h["k"] // 4]
    assert later  # a live qx slot of a later stage of the same four-stage sweep
    assert any(int(sq.nb[h["j"]]) == 0 for h in later)  # whose own soft term goes to the same slots
    assert {(h["k"], h["j"]) for h in later} == {(1, 2), (5, 6)}
    assert any(h["j"] == h["k"] for h in hits)  # and one inside the writing stage's own block
    # worked by hand for stage 1 (nb 3, ns 6: block of 24 at 8, write at 8 + 12 + 12 + 3 = 35 ..): stage 2's block
    # (nb 0, ns 2: Qx 4 | qx 4) starts at 32, stage 3's at 40
    assert [(h["array"], h["j"], h["off"], h["live"]) for h in hits if h["k"] == 1] == \
        [("Qx", 2, 3, False), ("qx", 2, 0, True), ("qx", 2, 1, True), ("qx", 2, 2, False), ("qx", 2, 3, False),
         ("Qx", 3, 0, True)]


@pytest.mark.parametrize("name", NAMES)
def test_no_case_is_refused(name):
    hits, refused = SC.soft_stray_targets(SC.make(name, 0))
    assert not refused
    if name == "softonly":
        assert hits == []  # nb = 0 everywhere: every soft term goes to its own slot
    if name == "odd":
        assert any(h["array"] == "qx" and h["live"] and h["j"] == 6 for h in hits)


def test_refusal_shape_is_refused():
    sq = SC.refusal_shape()
    assert (sq.N, sq.nb.tolist(), sq.ns.tolist(), int(sq.nx[2])) == (2, [0, 0, 4], [0, 0, 4], 8)
    hits, refused = SC.soft_stray_targets(sq)
    assert refused
    assert [(h["array"], h["j"], h["off"]) for h in hits] == [("Zl", 2, o) for o in (4, 5, 6, 7)]


def test_a_write_into_an_earlier_stage_zl_is_not_refused():
    """x0_box: stage 4's write passes the end of the Qx / qx carve into Zl of stage 0, which this pass has already
    read -- the same memory in the product (one flat block), so it is reproduced, not refused."""
    hits, refused = SC.soft_stray_targets(SC.make("x0_box", 0))
    assert not refused and any(h["array"] == "Zl" and h["j"] == 0 and h["k"] == 4 and h["live"] for h in hits)

"""Batched, device-resident soft-constraint IPM (hpmpc_mi355x_ipm_soft_batch, hk_soft_ipm) against the oracle.

Every comparison is per problem, against oracle.ipm_soft with k_max=50, mu0=100, mu_tol=1e-6, alpha_min=1e-8 at
helpers.TOL_SOFT (ux / t 5e-8, pi / lam 1e-6, stat 1e-7, relative to max(1, |ref|); kk and ret identical) -- the
comparison of tests/test_gpu_soft.py.  The batches were chosen so that the oracle's own rounding spread (its default
build against its FMA build) stays under those gates on every gated vector (worst case 12 % of the stat gate); the
oracle's iteration counts are pinned below, so a change of the inputs shows up as such.  Problem i of a mass-spring
batch has x0[0] = x0[1] = s_i; the rs_* batches are the admitted draws of tests/soft_cases.py (random stage
structure, spread at most 25 % of every gate by that module's admission rule, worst admitted 8.5 %).
"""
import numpy as np
import pytest

import soft_cases as SC
from helpers import TOL_SOFT
from hpmpc_amd.soft import (SoftBatchSolver, mass_spring_soft, soft_batch_layout, soft_plan_create)
from test_gpu_soft import _cmp

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
ARGS = dict(k_max=50, mu0=100.0, mu_tol=1e-6, alpha_min=1e-8)
assert ARGS == SC.ARGS
S5 = (0.2, 1.0, 2.0, 3.5, 6.0)


def _batch(scales, seeds=None, **mk):
    out = []
    for i, s in enumerate(scales):
        x0 = np.zeros(mk["nx"])
        x0[0] = x0[1] = s
        kw = dict(mk)
        if seeds is not None:
            kw["seed"] = seeds[i]
        out.append(mass_spring_soft(x0=x0, **kw))
    return out


# name -> (problems, the oracle's iteration counts)
FAMILIES = {
    # mixed exit iterations, a partial last stage quad, hard and soft boxes on the last stage
    "mixed_N4": (lambda: _batch(S5, N=4, nx=4, nu=2, hard_last=2, Q_diag=1.0), [5, 6, 8, 6, 6]),
    # time-variant data: every stage block differs between problems
    "tv_N8": (lambda: _batch(S5, seeds=[3 + i for i in range(5)], N=8, nx=8, nu=3, time_variant=True, Q_diag=1.0,
                             Zq=2.0, zl=5.0), [5, 6, 8, 8, 9]),
    # full tile (nu + nx = 16), the compiled inner-stage class
    "full_N9": (lambda: _batch((0.2, 1.0, 3.5), N=9, nx=12, nu=4, Q_diag=1.0, Zq=1.0), [5, 6, 10]),
    # shortest horizon
    "N1": (lambda: _batch((0.2, 1.0), N=1, nx=4, nu=2, Q_diag=1.0), [5, 6]),
}
# random stage structure (tests/soft_cases.py): the admitted draws of each case as one batch that shares sizes and idxb
FAMILIES.update({"rs_" + c: ((lambda c=c: SC.problems(c)), SC.kks(c)) for c in SC.CASES})
RS_ORDER = ("mixed_N4", "rs_odd", "rs_stray")  # rs_odd: two four-stage sweeps; rs_stray: stray writes into live qx


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's solutions, computed once per batch and shared (never modified)."""
    cache = {}

    def get(name, sqs=None, ux=None, **args):
        if name not in cache:
            sqs = FAMILIES[name][0]() if sqs is None else sqs
            a = dict(ARGS)
            a.update(args)
            cache[name] = (sqs, [oracle.ipm_soft(sq.copy(), **a, **({} if ux is None else dict(ux=ux)))
                                 for sq in sqs])
        return cache[name]

    return get


def _check(sqs, got, ref):
    assert len(got) == len(ref)
    for sq, g, r in zip(sqs, got, ref):
        _cmp(sq, g, r)


@pytest.mark.parametrize("name", list(FAMILIES), ids=list(FAMILIES))
def test_batch_vs_oracle(refs, name):
    sqs, ref = refs(name)
    assert [r["kk"] for r in ref] == FAMILIES[name][1], [r["kk"] for r in ref]
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    sv.ws.fill_(float("nan"))  # the workspace needs no initialisation
    sv.solve(**ARGS)
    got = sv.results()
    for i, (sq, g, r) in enumerate(zip(sqs, got, ref)):
        share = SC.gate_share(SC.soft_errors(sq, g, r))
        print(f"batch {name} problem {i}: kk {g['kk']} ret {g['ret']}, share of gate " +
              " ".join(f"{k} {v:.2e}" for k, v in share.items()))
    _check(sqs, got, ref)
    if name in ("mixed_N4", "rs_odd"):  # the waves retire at different iterations
        assert len({g["kk"] for g in got}) > 1


@pytest.mark.parametrize("name", RS_ORDER)
def test_sub_range(refs, name):
    sqs, ref = refs(name)
    last = len(sqs) - 1  # every problem but the first and the last: 1..3 of mixed_N4's and rs_odd's five
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    for x in (sv.ux, sv.pi, sv.lam, sv.t, sv.stat):
        x.fill_(-7.25)
    sv.kk.fill_(-3)
    sv.ret.fill_(-3)
    sv.solve(p0=1, count=last - 1, **ARGS)
    sv.torch.cuda.synchronize()
    for p in (0, last):
        for x in (sv.ux, sv.pi, sv.lam, sv.t, sv.stat):
            assert bool((x[p] == -7.25).all())
        assert int(sv.kk[p]) == -3 and int(sv.ret[p]) == -3
    got = sv.results()
    _check(sqs[1:last], got[1:last], ref[1:last])


def _stat_err(g, r):
    assert g["stat"].shape == r["stat"].shape
    return np.max(np.abs(g["stat"] - r["stat"]) / np.maximum(1.0, np.abs(r["stat"])))


def test_exit_k_max(refs):
    sqs, _ = refs("mixed_N4")
    _, ref = refs("mixed_N4_kmax3", sqs=sqs, k_max=3)
    sv = SoftBatchSolver(sqs, k_max=3)
    a = dict(ARGS, k_max=3)
    sv.solve(**a)
    for g, r in zip(sv.results(), ref):
        assert (g["ret"], g["kk"]) == (1, 3) and (r["ret"], r["kk"]) == (1, 3)
        assert _stat_err(g, r) <= TOL_SOFT["stat"]


def test_exit_alpha_min(refs):
    sqs, ref = refs("alpha_min_N5", sqs=[mass_spring_soft(N=5, nx=4, nu=2, Q_diag=1.0)], alpha_min=0.9)
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    sv.solve(**dict(ARGS, alpha_min=0.9))
    for g, r in zip(sv.results(), ref):
        assert (g["ret"], g["kk"]) == (2, 1) and (r["ret"], r["kk"]) == (2, 1)
        assert _stat_err(g, r) <= TOL_SOFT["stat"]


def test_warm_start(refs):
    sqs = _batch((0.2, 2.0), N=5, nx=4, nu=2, Q_diag=1.0)
    rng = np.random.default_rng(4)
    ux0 = [0.05 * rng.standard_normal(sqs[0].nux(k) + 4) for k in range(sqs[0].N + 1)]
    _, ref = refs("warm_N5", sqs=sqs, ux=ux0, warm_start=1)
    assert [r["kk"] for r in ref] == [5, 9]
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    sv.set_ux([ux0] * len(sqs))
    sv.solve(warm_start=1, **ARGS)
    _check(sqs, sv.results(), ref)


@pytest.mark.parametrize("name", RS_ORDER)
def test_agrees_with_single_problem_entry_point(product, refs, name):
    """kk / ret of d_ip2_mpc_soft_tv per problem; the vectors to TOL_SOFT (the fused kernel may contract products
    differently, so bitwise equality is not required)."""
    sqs, _ = refs(name)
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    sv.solve(**ARGS)
    got = sv.results()
    _check(sqs, got, [product.ipm_soft(sq.copy(), **ARGS) for sq in sqs])


def _share_tail(sqs):
    """The draws of a random-structure case differ in every stage, so they cannot share blocks as they are: stage 0
    of each draw in front of the stages >= 1 of the first (BAbt / RSQrq; d, Z, z stay per problem).  These hybrids are
    no admitted draws; the test that uses them compares the product with itself, bitwise."""
    out = []
    for sq in sqs:
        h = sqs[0].copy()
        h.BAbt[0], h.RSQrq[0] = sq.BAbt[0].copy(), sq.RSQrq[0].copy()
        h.d, h.Z, h.z = [a.copy() for a in sq.d], [a.copy() for a in sq.Z], [a.copy() for a in sq.z]
        out.append(h)
    return out


@pytest.mark.parametrize("name", RS_ORDER)
def test_shared_layout_bitwise(refs, name):
    sqs, _ = refs(name)
    if name != "mixed_N4":
        sqs = _share_tail(sqs)
    out = []
    for shared in (False, True):
        sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"], shared=shared)
        sv.solve(**ARGS)
        sv.torch.cuda.synchronize()
        out.append([x.cpu().numpy().copy() for x in (sv.ux, sv.pi, sv.lam, sv.t, sv.kk, sv.ret, sv.stat)])
    assert out[0][4].max() > 0
    for a, b in zip(*out):
        assert np.array_equal(a, b)


def test_refusals():
    plan, err = soft_plan_create(mass_spring_soft(6, 6, 2))  # b_k read outside BAbt_k
    assert plan is None and err == EUNSUPPORTED
    sq = mass_spring_soft(6, 8, 2)
    sq.ng = sq.ng.copy()
    sq.ng[3] = 1
    plan, err = soft_plan_create(sq)
    assert plan is None and err == EUNSUPPORTED


def test_refuses_stray_write_into_zl():
    """The reference's soft-gradient write of stage N would land in Zl_N, which the same pass reads later."""
    sq = SC.refusal_shape()
    assert SC.soft_stray_targets(sq)[1]
    plan, err = soft_plan_create(sq)
    assert plan is None and err == EUNSUPPORTED


def test_range_and_null_refusals():
    """hpmpc_mi355x_ipm_soft_batch on the smallest shape (N = 2, nx = 2, nu = 1, one box per stage, two problems):
    p0 < 0, p0 + count > nprob and a null required array return HPMPC_MI355X_EUNSUPPORTED and leave it in
    hpmpc_mi355x_last_error(); count == 0 returns 0 with last_error 0; nothing is written."""
    from hpmpc_amd.soft import _soft_lib

    sv = SoftBatchSolver([mass_spring_soft(N=2, nx=2, nu=1, soft=False)] * 2, k_max=5)
    L = _soft_lib()
    outs = (sv.ux, sv.pi, sv.lam, sv.t, sv.ws, sv.stat)
    for x in outs:
        x.fill_(-7.25)
    sv.kk.fill_(-3)
    sv.ret.fill_(-3)
    p = lambda x, given=True: x.data_ptr() if given else None

    def call(p0, count, ok=True):
        return L.hpmpc_mi355x_ipm_soft_batch(sv.plan, None, sv.nprob, p0, count, p(sv.BAbt), p(sv.RSQrq), None, None,
                                             p(sv.d), p(sv.ux), p(sv.pi), p(sv.lam, ok), p(sv.t), p(sv.ws), 5, 100.0,
                                             1e-6, 1e-8, 0, 1, p(sv.kk), p(sv.ret), p(sv.stat),
                                             sv.torch.cuda.current_stream(sv.dev).cuda_stream)

    for args in ((-1, 1), (1, 2), (0, 3), (2, 1), (0, 2, False)):
        assert call(*args) == EUNSUPPORTED, args
        assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED, args
    for args in ((0, 0), (2, 0), (0, 0, False)):  # an empty range asks for no array
        assert call(*args) == 0, args
        assert L.hpmpc_mi355x_last_error() == 0, args
    sv.torch.cuda.synchronize()
    for x in outs:
        assert bool((x == -7.25).all())
    assert sv.kk.tolist() == [-3, -3] and sv.ret.tolist() == [-3, -3]


def test_no_constraints_leaves_outputs():
    sqs = [mass_spring_soft(N=5, nx=4, nu=2, soft=False, hard=False)] * 2
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    for x in (sv.ux, sv.pi, sv.lam, sv.t, sv.stat):
        x.fill_(-7.25)
    sv.kk.fill_(-3)
    sv.ret.fill_(-3)
    sv.solve(**ARGS)
    sv.torch.cuda.synchronize()
    assert sv.kk.tolist() == [0, 0] and sv.ret.tolist() == [0, 0]
    for x in (sv.ux, sv.pi, sv.lam, sv.t, sv.stat):
        assert bool((x == -7.25).all())


@pytest.mark.parametrize("name", ["mixed_N4", "full_N9", "rs_odd", "rs_full16"])
def test_offsets_and_sizes(refs, name):
    sqs, _ = refs(name)
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    lay = soft_batch_layout(sqs[0])
    assert sv.sizes == lay["sizes"]
    assert np.array_equal(sv.offsets, np.stack([lay["oD"], lay["oZ"], lay["oC"]], axis=1))

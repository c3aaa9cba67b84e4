"""The batched KKT adjoint solve (hpmpc_mi355x_kkt_adjoint_batch, hpmpc_mi355x_ocp_adjoint_batch, hk_adj.hip; Python:
OcpBatchSolver.adjoint / adjoint_sets / x0_gradient / feedback_gain_adjoint, BatchSolver.kkt_adjoint) on the GPU.

References, preconditions and the gate are kkt_adjoint_cases': the reference adjoint of a problem is T_ref' g with
T_ref built column by column from oracle re-solves, every test on it asserts `usable`, and a comparison is gated at
max(TOL_IPM, 4 x the spread of the oracle's two builds on that problem and cotangent) relative to max(1, |ref|).
Everything that is not a comparison against the oracle is bitwise: linearity in the cotangent, independence of a set
from its neighbours and from the scratch, the padded core against the dense call.
"""
import numpy as np
import pytest

import kkt_adjoint_cases as AC
import kkt_tangent_cases as TC
import test_gpu_kkt_tangent as TT
from hpmpc_amd.ocp_batch import VEC_KEYS, adjoint_set_arrays, kkt_set_arrays, ocp_lib
from ocp_batch_cases import IO

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
SENTINEL = -7.25
COT = AC.OUT_KEYS
_same, _dev = TT._same, TT._dev


@pytest.fixture(scope="module")
def refs(oracle):
    return AC.AdjRefs(oracle)


def _solved(refs, case, seeds, order="C"):
    return TT._solved(refs.tan, case, seeds, order)


def _cots(refs, case, seed, nadj):
    """The problem's nadj cotangents as dense dicts: set 0 is kkt_adjoint_cases' own, the others fresh draws."""
    g0 = refs.cotangent(case, seed)[1]
    s = refs.sizes(case, seed)
    out = [g0]
    for r in range(1, nadj):
        g = np.random.default_rng((100 + seed, r)).standard_normal(sum(s[k] for k in COT))
        out.append(AC.split(g, s, COT))
    return out


def _dense_cot(sv, cots):
    """cots[p][r] (dense dicts) -> {key: device tensor (nprob, nadj, size)}"""
    return {key: _dev(sv, np.array([[g[key] for g in row] for row in cots], dtype=np.float64)) for key in COT}


def _padded_cot(sv, Ps, cots):
    """cots[p][r] -> device gux, gpi, glam, gt of shape (nprob, nadj, N+1, .)"""
    nadj = len(cots[0])
    arrs = adjoint_set_arrays([AC.per_stage(P, g) for P, row in zip(Ps, cots) for g in row])
    return tuple(_dev(sv, x.reshape((len(Ps), nadj) + x.shape[1:])) for x in arrs)


def _host(out, keys=VEC_KEYS):
    return {k: out[k].cpu().numpy().copy() for k in keys if k in out}


def _fill(sv, nadj, value, scratch=float("nan")):
    for x in sv.grad_buffers(nadj).values():
        x.fill_(value)
    bufs = sv.kkt_buffers(nadj)
    for n in ("ux", "pi", "lam", "t"):
        bufs[n].fill_(value)
    bufs["scratch"].fill_(scratch)


def _live(P):
    """Masks (N+1, 16), (N+1, 16), (N+1, 32) of the padded bbar / qbar / dbar slots that carry an element."""
    N = P["N"]
    mb, mq, md = np.zeros((N + 1, 16), bool), np.zeros((N + 1, 16), bool), np.zeros((N + 1, 32), bool)
    for k in range(N + 1):
        nb, ng = P["nb"][k], P["ng"][k]
        pnb, png = (nb + 3) // 4 * 4, (ng + 3) // 4 * 4
        mb[k, :(P["nx"][k + 1] if k < N else 0)] = True
        mq[k, :(P["nu"][k] if k < N else 0) + P["nx"][k]] = True
        for o, n in ((0, nb), (pnb, nb), (2 * pnb, ng), (2 * pnb + png, ng)):
            md[k, o:o + n] = True
    return mb, mq, md


def _grads_of(P, bbar, qbar, dbar):
    """Padded (N+1, 16 / 16 / 32) gradients -> the dense b, q, r, lb, ub, lg, ug of one set: the dense call's epilogue
    restated in numpy (the transpose of kkt_set_arrays' placement)."""
    N, nx, nu = P["N"], P["nx"], P["nu"]
    cat = lambda v: np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in v] + [np.zeros(0)])
    pnb = [(n + 3) // 4 * 4 for n in P["nb"]]
    png = [(n + 3) // 4 * 4 for n in P["ng"]]
    K = range(N + 1)
    out = dict(r=cat([qbar[k, :nu[k]] for k in range(N)]),
               q=cat([qbar[k, (nu[k] if k < N else 0):(nu[k] if k < N else 0) + nx[k]] for k in K]),
               lb=cat([dbar[k, :P["nb"][k]] for k in K]), ub=cat([dbar[k, pnb[k]:pnb[k] + P["nb"][k]] for k in K]),
               lg=cat([dbar[k, 2 * pnb[k]:2 * pnb[k] + P["ng"][k]] for k in K]),
               ug=cat([dbar[k, 2 * pnb[k] + png[k]:2 * pnb[k] + png[k] + P["ng"][k]] for k in K]))
    if bbar is not None:
        out["b"] = cat([bbar[k, :nx[k + 1]] for k in range(N)])
    return out


# ------------------------------------------------------------------ 1: against the reference, dense and padded
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", AC.CASES)
def test_adjoint_matches_the_reference(refs, case, order):
    seeds = refs.usable(case)
    sv, Ps = _solved(refs, case, seeds, order)
    cots = [_cots(refs, case, s, 1) for s in seeds]
    _fill(sv, 1, float("nan"))
    got = _host(sv.adjoint(_dense_cot(sv, cots), 1))
    worst = 0.0
    for p, seed in enumerate(seeds):
        ref, alt = refs.adjoint(case, seed)
        gate = refs.gate(ref, alt)
        for key in VEC_KEYS:
            assert got[key][p, 0].shape == ref[key].shape, (case, key)
            err = AC.rel(got[key][p, 0], ref[key])
            worst = max(worst, err)
            assert err <= gate, (case, order, seed, key, err, gate)
    print(case, order, "worst relative error", worst)
    # the padded core computes the same numbers: the dense call's placements restated in numpy, element for element
    _fill(sv, 1, float("nan"))
    pad = [x.cpu().numpy() for x in sv.adjoint_sets(*_padded_cot(sv, Ps, cots), 1)]
    for p, P in enumerate(Ps):
        want = _grads_of(P, pad[0][p, 0], pad[1][p, 0], pad[2][p, 0])
        for key in VEC_KEYS:
            assert _same(got[key][p, 0], want[key]), (case, order, p, key)
        # and every padded element is written: padding as zeros
        for x, m in zip(pad, _live(P)):
            assert np.isfinite(x[p, 0]).all() and not x[p, 0][~m].any()


# ----------------------------------------------------------------------------- 2: exactly linear, no base leak
@pytest.mark.parametrize("case", ["V", "F", "H", "E"])
def test_adjoint_is_exactly_linear(refs, case):
    seeds = refs.usable(case)[:5]
    sv, Ps = _solved(refs, case, seeds)
    scale = lambda g, a: {k: a * v for k, v in g.items()}
    cots = [[g, scale(g, 2.0), scale(g, 0.0)] for g in (_cots(refs, case, s, 1)[0] for s in seeds)]
    _fill(sv, 3, float("nan"))
    got = _host(sv.adjoint(_dense_cot(sv, cots), 3))
    for key in VEC_KEYS:
        assert np.isfinite(got[key]).all()
        assert _same(got[key][:, 1], 2.0 * got[key][:, 0]), (case, key)
        assert not got[key][:, 2].any(), (case, key)
    assert max(np.abs(got["lb"][:, 0]).max(), np.abs(got["q"][:, 0]).max()) > 1e-3
    # all-null cotangents: zero gradients (dense and padded)
    _fill(sv, 3, float("nan"))
    zero = _host(sv.adjoint({}, 3))
    pad = sv.adjoint_sets(None, None, None, None, 3)
    sv.torch.cuda.synchronize()
    assert all(not zero[key].any() for key in VEC_KEYS) and all(not bool(x.any()) for x in pad)


# --------------------------------------------------------- 3: a set does not depend on its neighbours or the scratch
def test_sets_are_independent_and_only_the_range_is_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    cots = [_cots(refs, case, s, 5) for s in seeds]
    _fill(sv, 5, float("nan"))
    five = _host(sv.adjoint(_dense_cot(sv, cots), 5))
    pcot = _padded_cot(sv, Ps, cots)
    pad5 = [x.cpu().numpy().copy() for x in sv.adjoint_sets(*pcot, 5)]
    for r in (0, 2, 4):
        _fill(sv, 1, float("nan"))
        one = _host(sv.adjoint(_dense_cot(sv, [[row[r]] for row in cots]), 1))
        for key in VEC_KEYS:
            assert _same(one[key][:, 0], five[key][:, r]), (key, r)
    # a sub-range: problems 1, 2 of 4; everything outside keeps the sentinel, the scratch starts as NaN
    _fill(sv, 5, SENTINEL)
    part = _host(sv.adjoint(_dense_cot(sv, cots), 5, p0=1, count=2))
    for key in VEC_KEYS:
        assert _same(part[key][1:3], five[key][1:3]), key
        for p in (0, 3):
            assert _same(part[key][p], np.full_like(part[key][p], SENTINEL)), (key, p)
    _fill(sv, 5, SENTINEL)
    padp = [x.cpu().numpy().copy() for x in sv.adjoint_sets(*pcot, 5, p0=1, count=2)]
    scr = sv.kkt_buffers(5)["scratch"].cpu().numpy()
    for a, b in zip(padp, pad5):
        assert _same(a[1:3], b[1:3])
        for p in (0, 3):
            assert _same(a[p], np.full_like(a[p], SENTINEL))
    assert np.isnan(scr[0]).all() and np.isnan(scr[3]).all()  # the scratch of the other problems' sets is not touched


# -------------------------------------------------------------------------------- 4: the call writes no input
def test_inputs_and_workspace_are_not_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    P2 = [IO.new_rhs(P, seed=TC.RSEED) for P in Ps]
    b, q, d = (_dev(sv, x.reshape((len(Ps), 1) + x.shape[1:])) for x in kkt_set_arrays(P2))
    before_sets = [x.cpu().numpy().copy() for x in sv.kkt_sets(b, q, d, nrhs=1)]
    cots = [_cots(refs, case, s, 1) for s in seeds]
    dense = _dense_cot(sv, cots)
    pcot = _padded_cot(sv, Ps, cots)
    inputs = [sv.ws, sv.BAbt, sv.RSQrq, sv.DCt, sv.d] + list(pcot) + [dense[k] for k in COT]
    before = [x.cpu().numpy().copy() for x in inputs]
    sv.adjoint(dense, 1)
    sv.adjoint_sets(*pcot, 1)
    sv.torch.cuda.synchronize()
    for x, want in zip(inputs, before):
        assert _same(x.cpu().numpy(), want)
    after_sets = [x.cpu().numpy().copy() for x in sv.kkt_sets(b, q, d, nrhs=1)]
    for a, w in zip(after_sets, before_sets):
        assert _same(a, w)


# ------------------------------------------------------------------------------------- 5: a null bbar / gb
def test_without_b_the_rest_is_unchanged_and_b_is_not_touched(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    cots = [_cots(refs, case, s, 1) for s in seeds]
    dense, pcot = _dense_cot(sv, cots), _padded_cot(sv, Ps, cots)
    full = _host(sv.adjoint(dense, 1))
    pfull = [x.cpu().numpy().copy() for x in sv.adjoint_sets(*pcot, 1)]
    assert full["b"].any() and pfull[0].any()
    rest = tuple(k for k in VEC_KEYS if k != "b")
    _fill(sv, 1, SENTINEL)
    nob = _host(sv.adjoint(dense, 1, want=rest))
    assert set(nob) == set(rest)
    for key in rest:
        assert _same(nob[key], full[key]), key
    gb = sv.grad_buffers(1)["b"].cpu().numpy()
    assert _same(gb, np.full_like(gb, SENTINEL))
    _fill(sv, 1, SENTINEL)
    bbar, qbar, dbar = sv.adjoint_sets(*pcot, 1, want_b=False)
    assert bbar is None
    assert _same(qbar.cpu().numpy(), pfull[1]) and _same(dbar.cpu().numpy(), pfull[2])
    pi = sv.kkt_buffers(1)["pi"].cpu().numpy()
    assert _same(pi, np.full_like(pi, SENTINEL))


# ------------------------------------------------------------------------------------------- 6: the feedback gain
@pytest.mark.parametrize("case,nx0,shape", TT.GAIN_CASES, ids=[c[0] for c in TT.GAIN_CASES])
def test_feedback_gain_adjoint_against_the_oracle(refs, case, nx0, shape):
    seeds = refs.usable(case)
    sv, Ps = _solved(refs, case, seeds)
    nu0, nx1 = Ps[0]["nu"][0], Ps[0]["nx"][1]
    assert Ps[0]["nx"][0] == 0 and (nu0, nx1) == shape
    rng = np.random.default_rng(11)
    A0, S0 = rng.standard_normal((len(Ps), nx1, nx0)), rng.standard_normal((len(Ps), nu0, nx0))
    K = sv.feedback_gain_adjoint(A0, S0).cpu().numpy()
    assert K.shape == (len(Ps), nu0, nx0)
    worst = 0.0
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        for i in range(nx0):
            D = {k: P[k] for k in ("N", "nx", "nu", "nb", "ng")}
            D["b"] = [A0[p][:, i]] + [np.zeros_like(v) for v in P["b"][1:]]
            D["r"] = [S0[p][:, i]] + [np.zeros_like(v) for v in P["r"][1:]]
            ref, alt = refs.tan.tangent_of(case, seed, D, ("x0", i))
            gate = refs.tan.gate(ref, alt)
            err = TC.rel(K[p, :, i], ref["u"][:nu0])
            worst = max(worst, err)
            assert err <= gate, (case, seed, i, err, gate)
    print("gain", case, "worst relative error", worst)
    # a gain shared by every problem: (nx1, nx0) / (nu0, nx0) blocks
    K1 = sv.feedback_gain_adjoint(A0[0], S0[0]).cpu().numpy()
    assert _same(K1[0], K[0])
    # x0_gradient is the chain rule on the call's own outputs.  Its sum has nx1 + nu0 = 11 (H: 16) products, so it
    # agrees with numpy's to that many roundings of the absolute sum, whatever the summation order, and a rounding is
    # eps / 2: within 16 eps (|A0|' |gb_0| + |S0|' |gr_0|)
    gu = np.zeros((len(Ps), nu0, sv.sizes["u"]))
    gu[:, np.arange(nu0), np.arange(nu0)] = 1.0
    grads = sv.adjoint({"u": _dev(sv, gu)}, nu0, want=("b", "r"))
    got = sv.x0_gradient(A0, S0, grads).cpu().numpy()
    gb, gr = grads["b"].cpu().numpy()[:, :, :nx1], grads["r"].cpu().numpy()[:, :, :nu0]
    want = np.einsum("pji,prj->pri", A0, gb) + np.einsum("pji,prj->pri", S0, gr)
    bound = 16 * np.finfo(np.float64).eps * (np.einsum("pji,prj->pri", np.abs(A0), np.abs(gb)) +
                                             np.einsum("pji,prj->pri", np.abs(S0), np.abs(gr)))
    assert got.shape == (len(Ps), nu0, nx0) and (np.abs(got - want) <= bound).all()
    assert _same(got, K)


# -------------------------------------------------------------------------------------------------- 7: refusals
def test_refusals_write_nothing(refs):
    case = "V"
    seeds = refs.usable(case)[:3]
    sv, Ps = _solved(refs, case, seeds)
    assert sv.sizes["DCt"] > 0
    cots = [_cots(refs, case, s, 1) for s in seeds]
    dense, (gux, gpi, glam, gt) = _dense_cot(sv, cots), _padded_cot(sv, Ps, cots)
    _fill(sv, 1, SENTINEL, scratch=SENTINEL)
    bufs, grads = sv.kkt_buffers(1), sv.grad_buffers(1)
    L = ocp_lib()
    tile = L.hpmpc_mi355x_ocp_tile_plan(sv.plan)
    ptr = lambda x, given=True: x.data_ptr() if given else None

    def core(nadj=1, p0=0, count=3, DCt=True, scratch=True, ws=True, qbar=True, dbar=True, mats=True):
        return L.hpmpc_mi355x_kkt_adjoint_batch(
            tile, None, sv.nprob, p0, count, nadj, ptr(sv.BAbt, mats), ptr(sv.RSQrq), ptr(sv.DCt, DCt), ptr(gux),
            ptr(gpi), ptr(glam), ptr(gt), ptr(bufs["pi"]), ptr(bufs["ux"], qbar), ptr(bufs["lam"], dbar),
            ptr(sv.ws, ws), ptr(bufs["scratch"], scratch), sv._stream())

    def ocp(nadj=1, p0=0, count=3, plan=True, outs=True, scratch=True, ws=True, DCt=True):
        return L.hpmpc_mi355x_ocp_adjoint_batch(
            sv.plan if plan else None, sv.nprob, p0, count, nadj, ptr(sv.BAbt), ptr(sv.RSQrq), ptr(sv.DCt, DCt),
            *(ptr(dense[k]) for k in COT), *(ptr(grads[k], outs) for k in VEC_KEYS), ptr(sv.ws, ws),
            ptr(bufs["scratch"], scratch), sv._stream())

    calls = [core(nadj=0), core(nadj=-1), core(scratch=False), core(ws=False), core(qbar=False), core(dbar=False),
             core(DCt=False), core(mats=False), core(p0=1, count=3), core(p0=-1, count=1), core(nadj=2 ** 30),
             ocp(nadj=0), ocp(plan=False), ocp(outs=False), ocp(scratch=False), ocp(ws=False), ocp(DCt=False),
             ocp(p0=2, count=2), ocp(p0=-1, count=1), ocp(nadj=2 ** 30)]
    for i, rc in enumerate(calls):
        assert rc == EUNSUPPORTED, i
    assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    assert core(count=0) == 0 and ocp(count=0) == 0 and core(count=0, qbar=False) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    for x in list(grads.values()) + list(bufs.values()):
        h = x.cpu().numpy()
        assert _same(h, np.full_like(h, SENTINEL))
    with pytest.raises(ValueError):
        sv.adjoint(dense, 2)  # the tensors hold one cotangent per problem
    with pytest.raises(ValueError):
        sv.adjoint(dense, 1, want=())  # the dense call needs at least one output
    with pytest.raises(ValueError):
        sv.adjoint(dict(dense, A=sv.BAbt), 1)  # cotangents are u, x, pi, lam, t


# ------------------------------------------------------------------------------------ 8: the plain batched route
def test_batch_solver_route(refs):
    from hpmpc_amd.batch import BatchSolver
    from test_gpu_kkt_batch import _batched_qp

    case = "V0"
    seeds = refs.usable(case)
    Ps = [refs.ipm(case, s)[0] for s in seeds]
    s = BatchSolver(_batched_qp(Ps), k_max=TC.K_MAX)
    s.ipm(**TC.TIGHT)
    s.torch.cuda.synchronize()
    assert s.kk.tolist() == [refs.ipm(case, sd)[1]["kk"] for sd in seeds]
    cots = [_cots(refs, case, sd, 1) for sd in seeds]
    s.kkt_buffers(1)["scratch"].fill_(float("nan"))
    pad = [x.cpu().numpy() for x in s.kkt_adjoint(*_padded_cot(s, Ps, cots), 1)]
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        ref, alt = refs.adjoint(case, seed)
        got = _grads_of(P, pad[0][p, 0], pad[1][p, 0], pad[2][p, 0])
        assert AC.grad_err(got, ref) <= refs.gate(ref, alt), seed

"""The OCP matrix gradients (hpmpc_mi355x_ocp_matrix_grads_batch, hpmpc_mi355x_ocp_adjoint_data_batch, hk_matgrad.hip;
Python: OcpBatchSolver.matrix_gradients / adjoint_data) on the GPU.

References, preconditions and the gate are kkt_matgrad_cases': the reference gradient of a matrix element is
g' T_ref dF with dF the oracle's residual difference for that element, every test on it asserts `usable`, and a
comparison is gated at max(TOL_IPM, 4 x the spread of the oracle's two builds on that problem) relative to
max(1, |ref|); the vector keys keep kkt_adjoint_cases' reference and gate.  Everything that is not a comparison against
the oracle is bitwise: the combined call against adjoint() and adjoint_sets() -> matrix_gradients(), the symmetry of
gQ / gR, linearity in the cotangent, independence of a set from its neighbours.
"""
import ctypes as C

import numpy as np
import pytest

import kkt_adjoint_cases as AC
import kkt_matgrad_cases as MC
import test_gpu_kkt_adjoint as AT
from hpmpc_amd.ocp_batch import KEYS, MAT_KEYS, VEC_KEYS, _OcpGrads, ocp_lib, unflatten_problems

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
SENTINEL = -7.25
COT = AC.OUT_KEYS
_same, _dev, _host = AT._same, AT._dev, AT._host


@pytest.fixture(scope="module")
def refs(oracle):
    return MC.shared(oracle)


def _solved(refs, case, seeds, order="C"):
    return AT._solved(refs.adj, case, seeds, order)


def _cots(refs, case, seed, nadj):
    return AT._cots(refs.adj, case, seed, nadj)


def _fill(sv, nadj, value, scratch=float("nan")):
    for x in list(sv.grad_buffers(nadj).values()) + list(sv.matrix_grad_buffers(nadj).values()):
        x.fill_(value)
    bufs = sv.kkt_buffers(nadj)
    for n in ("ux", "pi", "lam", "t"):
        bufs[n].fill_(value)
    bufs["scratch"].fill_(scratch)


def _all_buffers(sv, nadj):
    return dict(sv.grad_buffers(nadj), **sv.matrix_grad_buffers(nadj))


# ------------------------------------------------------------------ 1: against the reference, every key, both orders
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", MC.CASES)
def test_adjoint_data_matches_the_reference(refs, case, order):
    seeds = refs.usable(case)
    sv, Ps = _solved(refs, case, seeds, order)
    cots = [_cots(refs, case, s, 1) for s in seeds]
    _fill(sv, 1, float("nan"))
    out = sv.adjoint_data(AT._dense_cot(sv, cots), 1)
    assert tuple(out) == KEYS
    got = _host(out, KEYS)
    worst = 0.0
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        ref, alt = refs.gradients(case, seed)
        gate = refs.gate(ref, alt)
        want = MC.flat(P, ref, order)
        for key in MAT_KEYS:
            assert got[key][p, 0].shape == want[key].shape == (sv.sizes[key],), (case, key)
            assert np.isfinite(got[key][p, 0]).all(), (case, order, seed, key)
            err = AC.rel(got[key][p, 0], want[key])
            worst = max(worst, err)
            print(case, order, seed, key, err, gate)
            assert err <= gate, (case, order, seed, key, err, gate)
        vref, valt = refs.adj.adjoint(case, seed)
        vgate = refs.adj.gate(vref, valt)
        for key in VEC_KEYS:
            assert got[key][p, 0].shape == vref[key].shape, (case, key)
            assert AC.rel(got[key][p, 0], vref[key]) <= vgate, (case, order, seed, key)
    print(case, order, "worst relative error of the matrix gradients", worst)


# --------------------------------- 2, 3: the combined call is the two calls it is made of; gQ and gR are symmetric
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", ["V", "F", "H", "E"])
def test_combined_call_is_bitwise_its_parts_and_symmetric(refs, case, order):
    seeds = refs.adj.usable(case)[:4]  # bitwise only: no matrix-gradient reference is needed
    sv, Ps = _solved(refs, case, seeds, order)
    cots = [_cots(refs, case, s, 2) for s in seeds]
    dense = AT._dense_cot(sv, cots)
    _fill(sv, 2, float("nan"))
    got = _host(sv.adjoint_data(dense, 2), KEYS)
    _fill(sv, 2, float("nan"))
    vec = _host(sv.adjoint(dense, 2))
    for key in VEC_KEYS:
        assert _same(got[key], vec[key]), (case, key)
    _fill(sv, 2, float("nan"))
    bbar, qbar, dbar = sv.adjoint_sets(*AT._padded_cot(sv, Ps, cots), 2)
    mat = _host(sv.matrix_gradients(bbar, qbar, dbar, 2), MAT_KEYS)
    for key in MAT_KEYS:
        assert np.isfinite(mat[key]).all() and _same(got[key], mat[key]), (case, key)
    P = Ps[0]
    for r in range(2):
        blocks = unflatten_problems({k: got[k][:, r] for k in MC.SYM_KEYS}, P["N"], P["nx"], P["nu"], P["nb"], P["ng"],
                                    order, keys=list(MC.SYM_KEYS))
        for per in blocks:
            for key in MC.SYM_KEYS:
                assert all(_same(M, M.T) for M in per[key]), (case, key)
        assert max(np.abs(M - np.diag(np.diag(M))).max() for per in blocks for M in per["Q"] if M.size) > 1e-3


# ------------------------------------------------------------------------------------ 4: exactly linear
def test_doubling_the_cotangents_doubles_every_gradient(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    scale = lambda g, a: {k: a * v for k, v in g.items()}
    cots = [[g, scale(g, 2.0)] for g in (_cots(refs, case, s, 1)[0] for s in seeds)]
    _fill(sv, 2, float("nan"))
    got = _host(sv.adjoint_data(AT._dense_cot(sv, cots), 2), KEYS)
    for key in KEYS:
        assert np.isfinite(got[key]).all() and _same(got[key][:, 1], 2.0 * got[key][:, 0]), key
    assert min(np.abs(got[key][:, 0]).max() for key in MAT_KEYS) > 1e-3


# --------------------------------------------------------- 5: a set does not depend on its neighbours; ranges and want
def test_sets_are_independent_and_only_the_range_and_want_are_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    cots = [_cots(refs, case, s, 3) for s in seeds]
    dense = AT._dense_cot(sv, cots)
    _fill(sv, 3, float("nan"))
    three = _host(sv.adjoint_data(dense, 3), KEYS)
    for r in (0, 2):
        _fill(sv, 1, float("nan"))
        one = _host(sv.adjoint_data(AT._dense_cot(sv, [[row[r]] for row in cots]), 1), KEYS)
        for key in KEYS:
            assert _same(one[key][:, 0], three[key][:, r]), (key, r)
    # problems 1, 2 of 4 and five of the fourteen arrays: everything else keeps the sentinel
    want = ("A", "b", "Q", "lb", "C")
    _fill(sv, 3, SENTINEL)
    part = sv.adjoint_data(dense, 3, want=want, p0=1, count=2)
    assert tuple(part) == want
    for key, x in _all_buffers(sv, 3).items():
        h = x.cpu().numpy()[..., :max(sv.sizes[key], 1)]
        if key in want:
            assert _same(h[1:3, :, :sv.sizes[key]], three[key][1:3]), key
            h = h[[0, 3]]
        assert _same(h, np.full_like(h, SENTINEL)), key
    # the core alone, on the padded adjoint solution of the range
    _fill(sv, 3, SENTINEL)
    bbar, qbar, dbar = sv.adjoint_sets(*AT._padded_cot(sv, Ps, cots), 3)
    core = _host(sv.matrix_gradients(bbar, qbar, dbar, 3, want=("B", "D"), p0=2, count=1), ("B", "D"))
    for key, x in sv.matrix_grad_buffers(3).items():
        h = x.cpu().numpy()
        if key in core:
            assert _same(core[key][2], three[key][2]), key
            h = h[[0, 1, 3]]
        assert _same(h, np.full_like(h, SENTINEL)), key


# -------------------------------------------------------------------------------- 6: the call writes no input
def test_inputs_and_workspace_are_not_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    cots = [_cots(refs, case, s, 1) for s in seeds]
    dense = AT._dense_cot(sv, cots)
    pcot = AT._padded_cot(sv, Ps, cots)
    bbar, qbar, dbar = (x.clone() for x in sv.adjoint_sets(*pcot, 1))
    inputs = [sv.ws, sv.BAbt, sv.RSQrq, sv.DCt, sv.d, sv.ux, sv.pi, sv.lam, sv.t, bbar, qbar, dbar] + \
        [dense[k] for k in COT]
    before = [x.cpu().numpy().copy() for x in inputs]
    sv.adjoint_data(dense, 1)
    sv.matrix_gradients(bbar, qbar, dbar, 1)
    sv.torch.cuda.synchronize()
    for x, want in zip(inputs, before):
        assert _same(x.cpu().numpy(), want)


# ------------------------------------------------------------------------ 7: one array alone; A without b
def test_single_arrays_run_and_a_forces_the_multiplier_half(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    cots = [_cots(refs, case, s, 1) for s in seeds]
    dense = AT._dense_cot(sv, cots)
    full = _host(sv.adjoint_data(dense, 1), KEYS)
    for key in ("Q", "A"):
        _fill(sv, 1, SENTINEL)
        one = sv.adjoint_data(dense, 1, want=(key,))
        assert tuple(one) == (key,) and _same(one[key].cpu().numpy(), full[key]), key
        for other, x in _all_buffers(sv, 1).items():  # gb among them: not wanted, not written
            if other != key:
                h = x.cpu().numpy()
                assert _same(h, np.full_like(h, SENTINEL)), (key, other)
    assert np.abs(full["A"]).max() > 1e-3
    # another base iterate: the gradients follow it (pi enters gA linearly with qxbar)
    base = dict(ux=sv.ux.clone(), pi=2.0 * sv.pi, lam=sv.lam.clone())
    moved = sv.adjoint_data(dense, 1, want=("A", "Q"), base=base)
    assert _same(moved["Q"].cpu().numpy(), full["Q"]) and not _same(moved["A"].cpu().numpy(), full["A"])


# -------------------------------------------------------------------------------------------------- 8: refusals
def test_refusals_write_nothing(refs):
    case = "V"
    seeds = refs.usable(case)[:3]
    sv, Ps = _solved(refs, case, seeds)
    assert sv.sizes["DCt"] > 0
    cots = [_cots(refs, case, s, 1) for s in seeds]
    dense = AT._dense_cot(sv, cots)
    bbar, qbar, dbar = (x.clone() for x in sv.adjoint_sets(*AT._padded_cot(sv, Ps, cots), 1))
    _fill(sv, 1, SENTINEL, scratch=SENTINEL)
    bufs, grads = sv.kkt_buffers(1), _all_buffers(sv, 1)
    L = ocp_lib()
    ptr = lambda x, given=True: x.data_ptr() if given else None

    def struct(want, stride=None):
        gs = _OcpGrads()
        for i, key in enumerate(KEYS):
            if key in want:
                gs.ptr[i], gs.stride[i] = grads[key].data_ptr(), grads[key].shape[-1] if stride is None else stride
        return gs

    def core(nadj=1, p0=0, count=3, plan=True, want=MAT_KEYS, gs=True, ux=True, pi=True, lam=True, b=True, q=True,
             d=True, stride=None):
        return L.hpmpc_mi355x_ocp_matrix_grads_batch(
            sv.plan if plan else None, sv.nprob, p0, count, nadj, ptr(sv.ux, ux), ptr(sv.pi, pi), ptr(sv.lam, lam),
            ptr(bbar, b), ptr(qbar, q), ptr(dbar, d), C.byref(struct(want, stride)) if gs else None, sv._stream())

    def both(nadj=1, p0=0, count=3, plan=True, want=KEYS, gs=True, ux=True, pi=True, lam=True, scratch=True, ws=True,
             DCt=True, stride=None):
        return L.hpmpc_mi355x_ocp_adjoint_data_batch(
            sv.plan if plan else None, sv.nprob, p0, count, nadj, ptr(sv.BAbt), ptr(sv.RSQrq), ptr(sv.DCt, DCt),
            ptr(sv.ux, ux), ptr(sv.pi, pi), ptr(sv.lam, lam), *(ptr(dense[k]) for k in COT),
            C.byref(struct(want, stride)) if gs else None, ptr(sv.ws, ws), ptr(bufs["scratch"], scratch), sv._stream())

    calls = [core(nadj=0), core(nadj=-1), core(nadj=2 ** 30), core(p0=1, count=3), core(p0=-1, count=1),
             core(plan=False), core(gs=False), core(want=()), core(want=("A", "b")), core(ux=False), core(q=False),
             core(pi=False), core(b=False), core(lam=False), core(d=False), core(want=("Q",), stride=1),
             both(nadj=0), both(nadj=2 ** 30), both(p0=2, count=2), both(p0=-1, count=1), both(plan=False),
             both(gs=False), both(want=()), both(ux=False), both(pi=False), both(lam=False), both(scratch=False),
             both(ws=False), both(DCt=False), both(want=("Q",), stride=1), both(want=("q",), stride=1)]
    for i, rc in enumerate(calls):
        assert rc == EUNSUPPORTED, i
    assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    assert core(count=0) == 0 and both(count=0) == 0 and core(count=0, q=False) == 0
    # what is not needed may be null: no pi / bbar without A and B, no lam / dbar without C and D
    assert core(want=("Q", "S", "R"), pi=False, b=False, lam=False, d=False) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    for key, x in list(grads.items()) + list(bufs.items()):
        if key not in ("Q", "S", "R"):
            h = x.cpu().numpy()
            assert _same(h, np.full_like(h, SENTINEL)), key
    with pytest.raises(ValueError):
        sv.adjoint_data(dense, 2)  # the tensors hold one cotangent per problem
    with pytest.raises(ValueError):
        sv.adjoint_data(dense, 1, want=())
    with pytest.raises(ValueError):
        sv.adjoint_data(dense, 1, want=("u",))
    with pytest.raises(ValueError):
        sv.matrix_gradients(bbar, qbar, dbar, 1, want=("b",))  # the vector gradients are adjoint()'s
    with pytest.raises(ValueError):
        sv.matrix_gradients(None, qbar, dbar, 1, want=("A",))

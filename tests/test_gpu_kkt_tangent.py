"""The batched KKT tangent solve (hpmpc_mi355x_kkt_tangent_batch, hpmpc_mi355x_ocp_tangent_batch, hk_tan.hip; Python:
OcpBatchSolver.tangent / tangent_sets / feedback_gain, BatchSolver.kkt_tangent) and the multi-set finish
(hpmpc_mi355x_ocp_unpack_sets; OcpBatchSolver.kkt_sets(dense=True)) on the GPU.

References, preconditions and the gate are kkt_tangent_cases': the reference tangent of a problem is the difference of
two oracle re-solves, every test on it asserts `usable`, and a comparison is gated at max(TOL_IPM, 4 x the spread of
the oracle's two builds on that problem and direction) relative to max(1, |ref|).  Everything that is not a
comparison against the oracle is bitwise: linearity in the direction, independence of a set from its neighbours and
from the scratch, the padded core against the dense call, the dense sets against resolve() -> finish().
"""
import numpy as np
import pytest

import kkt_tangent_cases as TC
from hpmpc_amd.ocp_batch import _OcpData, flatten_problems, kkt_set_arrays, ocp_lib, tangent_set_arrays
from ocp_batch_cases import IO, make_solver, pack_problems, to_device

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
SENTINEL = -7.25
OUT = TC.OUT_KEYS


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _same(a, b):
    return np.array_equal(_bits(a), _bits(b))


@pytest.fixture(scope="module")
def refs(oracle):
    return TC.TanRefs(oracle)


def _solved(refs, case, seeds, order="C"):
    """pack -> ocp_ipm_batch on the tightened problems; kk / ret equal the oracle's."""
    ipms = [refs.ipm(case, s) for s in seeds]
    Ps = [i[0] for i in ipms]
    sv = make_solver(Ps, order)
    pack_problems(sv, Ps)
    sv.solve(**TC.TIGHT)
    sv.torch.cuda.synchronize()
    assert sv.kk.tolist() == [i[1]["kk"] for i in ipms], case
    assert sv.ret.tolist() == [i[1]["ret"] for i in ipms], case
    assert min(sv.kk.tolist()) >= 1
    return sv, Ps


def _dev(sv, x):
    return sv.torch.from_numpy(np.ascontiguousarray(x)).to(sv.dev)


def _dirs(sv, deltas, ndir):
    """deltas[p][r] -> the dense direction tensors of OcpBatchSolver.tangent"""
    return {k: _dev(sv, v) for k, v in TC.flat_dirs(deltas, ndir).items()}


def _padded(sv, deltas, ndir):
    """deltas[p][r] -> device db, dq, dd of shape (nprob, ndir, N+1, .)"""
    arrs = tangent_set_arrays([D for row in deltas for D in row])
    return tuple(_dev(sv, x.reshape((len(deltas), ndir) + x.shape[1:])) for x in arrs)


def _host(out):
    return {k: out[k].cpu().numpy().copy() for k in OUT}


def _fill_outputs(sv, ndir, value, scratch=float("nan")):
    for x in sv.set_buffers(ndir).values():
        x.fill_(value)
    bufs = sv.kkt_buffers(ndir)
    for n in ("ux", "pi", "lam", "t"):
        bufs[n].fill_(value)
    bufs["scratch"].fill_(scratch)


# ------------------------------------------------------------------ 1: against the reference, dense and padded
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", TC.CASES)
def test_tangent_matches_the_reference(refs, case, order):
    seeds = refs.usable(case)
    sv, Ps = _solved(refs, case, seeds, order)
    deltas = [[refs.delta(case, s)] for s in seeds]
    _fill_outputs(sv, 1, float("nan"))
    got = _host(sv.tangent(_dirs(sv, deltas, 1), 1))
    worst = 0.0
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        ref, alt = refs.tangent(case, seed)
        gate = refs.gate(ref, alt)
        for key in OUT:
            assert got[key][p, 0].shape == ref[key].shape, (case, key)
            err = TC.rel(got[key][p, 0], ref[key])
            worst = max(worst, err)
            assert err <= gate, (case, order, seed, key, err, gate)
    print(case, order, "worst relative error", worst)
    # the padded core computes the same numbers: the dense call's placement restated in numpy, element for element
    db, dq, dd = _padded(sv, deltas, 1)
    pad = [x.cpu().numpy() for x in sv.tangent_sets(db, dq, dd, 1)]
    for p, P in enumerate(Ps):
        want = TC.dense_of(P, dict(ux=pad[0][p, 0], pi=pad[1][p, 0], lam=pad[2][p, 0], t=pad[3][p, 0]))
        for key in OUT:
            assert _same(got[key][p, 0], want[key]), (case, order, p, key)
    # and every padded element is written: padding as zeros
    N = sv.N
    for p, P in enumerate(Ps):
        for k in range(N + 1):
            nux, nx1 = P["nu"][k] + P["nx"][k], (P["nx"][k + 1] if k < N else 0)
            nc = 2 * ((P["nb"][k] + 3) // 4 * 4) + 2 * ((P["ng"][k] + 3) // 4 * 4)
            assert not pad[0][p, 0, k, nux:].any() and not pad[1][p, 0, k, nx1:].any()
            assert not pad[2][p, 0, k, nc:].any() and not pad[3][p, 0, k, nc:].any()


# ----------------------------------------------------------------------------- 2: exactly linear, no base leak
@pytest.mark.parametrize("case", ["V", "F", "H", "E"])
def test_tangent_is_exactly_linear(refs, case):
    seeds = refs.usable(case)[:5]
    sv, Ps = _solved(refs, case, seeds)
    deltas = [[D, TC.scaled(D, 2.0), TC.scaled(D, 0.0)] for D in (refs.delta(case, s) for s in seeds)]
    _fill_outputs(sv, 3, float("nan"))
    got = _host(sv.tangent(_dirs(sv, deltas, 3), 3))
    for key in OUT:
        assert np.isfinite(got[key]).all()
        assert _same(got[key][:, 1], 2.0 * got[key][:, 0]), (case, key)  # a difference of solves would round
        assert not got[key][:, 2].any(), (case, key)                      # a base leak would show here
    assert max(np.abs(got["lam"][:, 0]).max(), np.abs(got["u"][:, 0]).max()) > 1e-3
    # all-null directions: zero outputs (dense and padded)
    _fill_outputs(sv, 3, float("nan"))
    zero = _host(sv.tangent({}, 3))
    pad = sv.tangent_sets(None, None, None, 3)
    sv.torch.cuda.synchronize()
    assert all(not zero[key].any() for key in OUT) and all(not bool(x.any()) for x in pad)


# --------------------------------------------------------- 3: a set does not depend on its neighbours or the scratch
def test_sets_are_independent_and_only_the_range_is_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    deltas = [[refs.delta(case, s, rseed=TC.RSEED + r) for r in range(5)] for s in seeds]
    _fill_outputs(sv, 5, float("nan"))
    five = _host(sv.tangent(_dirs(sv, deltas, 5), 5))
    db, dq, dd = _padded(sv, deltas, 5)
    pad5 = [x.cpu().numpy().copy() for x in sv.tangent_sets(db, dq, dd, 5)]
    for r in (0, 2, 4):
        _fill_outputs(sv, 1, float("nan"))
        one = _host(sv.tangent(_dirs(sv, [[row[r]] for row in deltas], 1), 1))
        for key in OUT:
            assert _same(one[key][:, 0], five[key][:, r]), (key, r)
    # a sub-range: problems 1, 2 of 4; everything outside keeps the sentinel, the scratch starts as NaN
    _fill_outputs(sv, 5, SENTINEL)
    part = _host(sv.tangent(_dirs(sv, deltas, 5), 5, p0=1, count=2))
    for key in OUT:
        assert _same(part[key][1:3], five[key][1:3]), key
        for p in (0, 3):
            assert _same(part[key][p], np.full_like(part[key][p], SENTINEL)), (key, p)
    _fill_outputs(sv, 5, SENTINEL)
    padp = [x.cpu().numpy().copy() for x in sv.tangent_sets(db, dq, dd, 5, p0=1, count=2)]
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
    P2 = [[IO.new_rhs(P, seed=TC.RSEED)] for P in Ps]
    b, q, d = (_dev(sv, x.reshape((len(Ps), 1) + x.shape[1:])) for x in kkt_set_arrays([row[0] for row in P2]))
    before_sets = [x.cpu().numpy().copy() for x in sv.kkt_sets(b, q, d, nrhs=1)]
    deltas = [[refs.delta(case, s)] for s in seeds]
    dirs = _dirs(sv, deltas, 1)
    db, dq, dd = _padded(sv, deltas, 1)
    inputs = [sv.ws, sv.BAbt, sv.RSQrq, sv.DCt, sv.d, db, dq, dd] + [dirs[k] for k in sorted(dirs)]
    before = [x.cpu().numpy().copy() for x in inputs]
    sv.tangent(dirs, 1)
    sv.tangent_sets(db, dq, dd, 1)
    sv.torch.cuda.synchronize()
    for x, want in zip(inputs, before):
        assert _same(x.cpu().numpy(), want)
    after_sets = [x.cpu().numpy().copy() for x in sv.kkt_sets(b, q, d, nrhs=1)]
    for a, w in zip(after_sets, before_sets):
        assert _same(a, w)


# ------------------------------------------------------------------------------------------- 5: compute_mult = 0
def test_compute_mult_0_returns_zero_dpi(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    deltas = [[refs.delta(case, s)] for s in seeds]
    dirs = _dirs(sv, deltas, 1)
    full = _host(sv.tangent(dirs, 1))
    _fill_outputs(sv, 1, float("nan"))
    nomult = _host(sv.tangent(dirs, 1, compute_mult=0))
    assert full["pi"].any() and not nomult["pi"].any()
    assert _same(nomult["pi"], np.zeros_like(nomult["pi"]))  # +0.0, not -0.0
    for key in ("u", "x", "lam", "t"):
        assert _same(nomult[key], full[key]), key


# ------------------------------------------------------------------------------------------- 6: the feedback gain
# (case, nx0, (nu0, nx1)): F with three columns, and the (4, 12) class with the twelve of a full x_0
GAIN_CASES = [("F", 3, (3, 8)), ("H", 12, (4, 12))]


@pytest.mark.parametrize("case,nx0,shape", GAIN_CASES, ids=[c[0] for c in GAIN_CASES])
def test_feedback_gain_against_the_oracle(refs, case, nx0, shape):
    seeds = refs.usable(case)
    sv, Ps = _solved(refs, case, seeds)
    nu0, nx1 = Ps[0]["nu"][0], Ps[0]["nx"][1]
    assert Ps[0]["nx"][0] == 0 and (nu0, nx1) == shape
    rng = np.random.default_rng(11)
    A0, S0 = rng.standard_normal((len(Ps), nx1, nx0)), rng.standard_normal((len(Ps), nu0, nx0))
    K = sv.feedback_gain(A0, S0).cpu().numpy()
    assert K.shape == (len(Ps), nu0, nx0)
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        for i in range(nx0):
            D = {k: P[k] for k in ("N", "nx", "nu", "nb", "ng")}
            D["b"] = [A0[p][:, i]] + [np.zeros_like(v) for v in P["b"][1:]]
            D["r"] = [S0[p][:, i]] + [np.zeros_like(v) for v in P["r"][1:]]
            ref, alt = refs.tangent_of(case, seed, D, ("x0", i))
            gate = refs.gate(ref, alt)
            err = TC.rel(K[p, :, i], ref["u"][:nu0])
            assert err <= gate, (case, seed, i, err, gate)
    # a gain shared by every problem: (nx1, nx0) / (nu0, nx0) blocks
    K1 = sv.feedback_gain(A0[0], S0[0]).cpu().numpy()
    assert _same(K1[0], K[0])


# ------------------------------------------------------------------------------- 7: the multi-set dense finish
def test_dense_sets_are_resolve_then_finish(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    P2 = [[IO.new_rhs(P, seed=TC.RSEED + r) for r in range(3)] for P in Ps]
    # an equality input box: problem 1, set 2, stage 0, box 0 (an input: hidxb[0][0] < nu[0])
    assert Ps[1]["hidxb"][0][0] < Ps[1]["nu"][0]
    Q = P2[1][2]
    Q["ub"][0] = Q["ub"][0].copy()
    Q["ub"][0][0] = Q["lb"][0][0]
    b, q, d = (_dev(sv, x.reshape((len(Ps), 3) + x.shape[1:])) for x in kkt_set_arrays([P for row in P2 for P in row]))
    for x in sv.set_buffers(3).values():
        x.fill_(float("nan"))
    got = _host(sv.kkt_sets(b, q, d, nrhs=3, dense=True))
    for r in range(3):
        sv.resolve(to_device(sv, flatten_problems([row[r] for row in P2], "C")))
        want = sv.finish()
        sv.torch.cuda.synchronize()
        for key in OUT:
            assert _same(got[key][:, r], want[key].cpu().numpy()), (key, r)
    lb = Q["lb"][0][0]
    assert got["u"][1, 2, Ps[1]["hidxb"][0][0]] == lb  # the fix, from the set's own d
    # a sub-range leaves the other problems' sets alone
    for x in sv.set_buffers(3).values():
        x.fill_(SENTINEL)
    part = _host(sv.kkt_sets(b, q, d, nrhs=3, dense=True, p0=2, count=1))
    for key in OUT:
        assert _same(part[key][2], got[key][2])
        for p in (0, 1, 3):
            assert _same(part[key][p], np.full_like(part[key][p], SENTINEL))


# -------------------------------------------------------------------------------------------------- 8: refusals
def test_refusals_write_nothing(refs):
    case = "V"
    seeds = refs.usable(case)[:3]
    sv, Ps = _solved(refs, case, seeds)
    assert sv.sizes["DCt"] > 0
    deltas = [[refs.delta(case, s)] for s in seeds]
    dirs = _dirs(sv, deltas, 1)
    db, dq, dd = _padded(sv, deltas, 1)
    _fill_outputs(sv, 1, SENTINEL, scratch=SENTINEL)
    bufs, dense = sv.kkt_buffers(1), sv.set_buffers(1)
    L = ocp_lib()
    tile = L.hpmpc_mi355x_ocp_tile_plan(sv.plan)
    ptr = lambda x, given=True: x.data_ptr() if given else None

    def core(ndir=1, p0=0, count=3, DCt=True, scratch=True, ws=True, out=True):
        return L.hpmpc_mi355x_kkt_tangent_batch(
            tile, None, sv.nprob, p0, count, ndir, ptr(sv.BAbt), ptr(sv.RSQrq), ptr(sv.DCt, DCt), ptr(db), ptr(dq),
            ptr(dd), ptr(bufs["ux"], out), ptr(bufs["pi"]), ptr(bufs["lam"]), ptr(bufs["t"]), ptr(sv.ws, ws),
            ptr(bufs["scratch"], scratch), 1, sv._stream())

    def struct(matrix=None, stride=None):
        ds = _OcpData()
        for i, key in enumerate(("A", "B", "b", "Q", "S", "R", "q", "r", "lb", "ub", "C", "D", "lg", "ug")):
            if key in dirs:
                ds.ptr[i], ds.stride[i] = dirs[key].data_ptr(), (sv.sizes[key] if stride is None else stride)
            elif key == matrix:
                ds.ptr[i], ds.stride[i] = sv.BAbt.data_ptr(), 0
        return ds

    def ocp(ndir=1, p0=0, count=3, ds=None, given=True, out=True, scratch=True):
        import ctypes as C

        ds = struct() if ds is None else ds
        return L.hpmpc_mi355x_ocp_tangent_batch(
            sv.plan, C.byref(ds) if given else None, sv.nprob, p0, count, ndir, ptr(sv.BAbt), ptr(sv.RSQrq),
            ptr(sv.DCt), ptr(dense["u"], out), ptr(dense["x"]), ptr(dense["pi"]), ptr(dense["lam"]), ptr(dense["t"]),
            ptr(sv.ws), ptr(bufs["scratch"], scratch), 1, sv._stream())

    def sets(nrhs=1, p0=0, count=3, given=True):
        return L.hpmpc_mi355x_ocp_unpack_sets(
            sv.plan, sv.nprob, p0, count, nrhs, ptr(dd), ptr(bufs["ux"], given), ptr(bufs["pi"]), ptr(bufs["lam"]),
            ptr(bufs["t"]), ptr(dense["u"]), ptr(dense["x"]), ptr(dense["pi"]), ptr(dense["lam"]), ptr(dense["t"]),
            sv._stream())

    calls = [core(ndir=0), core(ndir=-1), core(scratch=False), core(ws=False), core(out=False), core(DCt=False),
             core(p0=1, count=3), core(p0=-1, count=1), core(ndir=2 ** 30),
             ocp(ndir=0), ocp(given=False), ocp(out=False), ocp(scratch=False), ocp(p0=2, count=2),
             ocp(ds=struct(matrix="A")), ocp(ds=struct(matrix="Q")), ocp(ds=struct(matrix="D")),
             ocp(ds=struct(stride=-1)),
             sets(nrhs=0), sets(given=False), sets(p0=3, count=1)]
    for i, rc in enumerate(calls):
        assert rc == EUNSUPPORTED, i
    assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    assert core(count=0) == 0 and ocp(count=0) == 0 and sets(count=0) == 0 and core(count=0, out=False) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    for x in list(dense.values()) + list(bufs.values()):
        h = x.cpu().numpy()
        assert _same(h, np.full_like(h, SENTINEL))
    with pytest.raises(ValueError):
        sv.tangent(dirs, 2)  # the tensors hold one direction per problem
    with pytest.raises(RuntimeError):
        sv.tangent(dict(dirs, A=sv.BAbt), 1)  # a matrix direction is refused by the library


# ------------------------------------------------------------------------------------ 9: the plain batched route
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
    deltas = [[refs.delta(case, sd)] for sd in seeds]
    db, dq, dd = _padded(s, deltas, 1)
    s.kkt_buffers(1)["scratch"].fill_(float("nan"))
    pad = [x.cpu().numpy() for x in s.kkt_tangent(db, dq, dd, 1)]
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        ref, alt = refs.tangent(case, seed)
        got = TC.dense_of(P, dict(ux=pad[0][p, 0], pi=pad[1][p, 0], lam=pad[2][p, 0], t=pad[3][p, 0]))
        assert TC.dense_err(got, ref) <= refs.gate(ref, alt), seed

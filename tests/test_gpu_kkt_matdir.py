"""The OCP matrix directions (hpmpc_mi355x_ocp_matrix_dirs_batch, hpmpc_mi355x_ocp_tangent_data_batch, hk_matdir.hip;
Python: OcpBatchSolver.matrix_directions / tangent_data) on the GPU.

References, preconditions and the gate are kkt_matdir_cases': the reference seed is the oracle's residual difference
for the drawn dtheta, the reference tangent the difference of two oracle re-solves on it, every test on them asserts
`usable`, and a comparison is gated at max(TOL_IPM, 4 x the spread of the oracle's two builds on that problem) relative
to max(1, |ref|).  Everything that is not a comparison against the oracle is bitwise: the combined call against
matrix_directions() -> tangent_sets(), against tangent() without matrices, linearity in the direction, independence
of a set from its neighbours.  The pairing with adjoint_data() is bounded by reference values and their gates only.
"""
import ctypes as C

import numpy as np
import pytest

import kkt_adjoint_cases as AC
import kkt_matdir_cases as DC
import kkt_matgrad_cases as MC
import kkt_tangent_cases as TC
import test_gpu_kkt_tangent as TT
from hpmpc_amd.ocp_batch import KEYS, MAT_KEYS, VEC_KEYS, _OcpData, flatten_sets, ocp_lib

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
SENTINEL = -7.25
OUT = TC.OUT_KEYS
_same, _dev = TT._same, TT._dev


@pytest.fixture(scope="module")
def refs(oracle):
    return DC.shared(oracle)


def _solved(refs, case, seeds, order="C"):
    return TT._solved(refs.tan, case, seeds, order)


def _direction(refs, case, seed, scale=1.0, keys=KEYS):
    """The problem's direction over `keys` in the interface form: dtheta (dQ, dR not symmetric) and the vector delta"""
    P = refs.ipm(case, seed)[0]
    D = {s: P[s] for s in AC.SIZE_KEYS}
    vec, mat = refs.tan.delta(case, seed), refs.dtheta(case, seed)
    for key in keys:
        D[key] = [scale * np.asarray(M) for M in (vec[key] if key in VEC_KEYS else mat[key])]
    return D


def _dirs(sv, sets, keys=KEYS):
    """sets[p][r] (interface-form directions) -> {key: device tensor (nprob, ndir, size)} in the solver's order"""
    return {k: _dev(sv, v) for k, v in flatten_sets(sets, len(sets[0]), keys, sv.order).items()}


def _host(out, keys=OUT):
    return {k: out[k].cpu().numpy().copy() for k in keys}


def _fill(sv, ndir, value, scratch=float("nan")):
    TT._fill_outputs(sv, ndir, value, scratch)
    for x in sv.direction_buffers(ndir).values():
        x.fill_(value)


def _core_dense(sv, Ps, dirs, ndir, **kw):
    """matrix_directions -> tangent_sets -> dense_of: the combined call rebuilt from its parts, per problem and set"""
    db, dq, dd = sv.matrix_directions(dirs, ndir, **kw)
    pad = [x.cpu().numpy() for x in sv.tangent_sets(db, dq, dd, ndir)]
    return [[TC.dense_of(P, dict(ux=pad[0][p, r], pi=pad[1][p, r], lam=pad[2][p, r], t=pad[3][p, r]))
             for r in range(ndir)] for p, P in enumerate(Ps)]


# ------------------------------------------------------------------ 1: against the reference; the call and its parts
@pytest.mark.parametrize("case,order", [("V", "C"), ("V", "F"), ("F", "C"), ("S", "C"), ("H", "C"), ("H", "F"),
                                        ("E", "C"), ("E", "F"), ("B", "C"), ("B", "F")])
def test_tangent_data_matches_the_reference(refs, case, order):
    seeds = refs.usable(case)
    sv, Ps = _solved(refs, case, seeds, order)
    dirs = _dirs(sv, [[_direction(refs, case, s)] for s in seeds])
    _fill(sv, 1, float("nan"))
    got = _host(sv.tangent_data(dirs, 1))
    worst = 0.0
    for p, seed in enumerate(seeds):
        ref, alt = refs.tangent(case, seed)
        gate = refs.gate(ref, alt)
        for key in OUT:
            assert got[key][p, 0].shape == ref[key].shape, (case, key)
            assert np.isfinite(got[key][p, 0]).all(), (case, order, seed, key)
            err = TC.rel(got[key][p, 0], ref[key])
            worst = max(worst, err)
            print(case, order, seed, key, err, gate)
            assert err <= gate, (case, order, seed, key, err, gate)
    print(case, order, "worst relative error of the tangent", worst)
    # the combined call is the core, the padded tangent solve and the dense placement, up to the padding
    _fill(sv, 1, float("nan"))
    parts = _core_dense(sv, Ps, dirs, 1)
    for p in range(len(Ps)):
        for key in OUT:
            assert _same(got[key][p, 0], parts[p][0][key]), (case, order, p, key)
    # and every element of the seed rows is written: padding as zeros
    rows = [x.cpu().numpy() for x in sv.direction_buffers(1).values()]
    assert all(np.isfinite(x).all() for x in rows)
    for p, P in enumerate(Ps):
        mb, mq, md = _live(P)
        for x, m in zip(rows, (mb, mq, md)):
            assert not x[p, 0][~m].any(), (case, p)


def _live(P):
    import test_gpu_kkt_adjoint as AT

    return AT._live(P)


# ------------------------------------------------------------------------------ 2: bitwise properties
def test_without_matrices_it_is_bitwise_tangent(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    dirs = _dirs(sv, [[_direction(refs, case, s, keys=VEC_KEYS), _direction(refs, case, s, -0.5, keys=VEC_KEYS)]
                      for s in seeds], VEC_KEYS)
    _fill(sv, 2, float("nan"))
    want = _host(sv.tangent(dirs, 2))
    _fill(sv, 2, float("nan"))
    got = _host(sv.tangent_data(dirs, 2))
    for key in OUT:
        assert np.isfinite(got[key]).all() and _same(got[key], want[key]), key
    assert np.abs(got["u"]).max() > 1e-3


def test_doubling_the_directions_doubles_every_output(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    dirs = _dirs(sv, [[_direction(refs, case, s), _direction(refs, case, s, 2.0)] for s in seeds])
    _fill(sv, 2, float("nan"))
    db, dq, dd = (x.cpu().numpy() for x in sv.matrix_directions(dirs, 2))
    for x in (db, dq, dd):
        assert np.isfinite(x).all() and _same(x[:, 1], 2.0 * x[:, 0])
    got = _host(sv.tangent_data(dirs, 2))
    for key in OUT:
        assert np.isfinite(got[key]).all() and _same(got[key][:, 1], 2.0 * got[key][:, 0]), key
    assert min(np.abs(got[key][:, 0]).max() for key in OUT) > 1e-3


def test_sets_are_independent_and_only_the_range_is_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    n = len(seeds)
    # set r of problem p: another problem's draw (the sizes are the case's), so the three sets differ
    sets = [[_direction(refs, case, seeds[(p + r) % n], 1.0 + r) for r in range(3)] for p in range(n)]
    dirs = _dirs(sv, sets)
    _fill(sv, 3, float("nan"))
    three = _host(sv.tangent_data(dirs, 3))
    rows3 = [x.cpu().numpy().copy() for x in sv.matrix_directions(dirs, 3)]
    for r in (0, 2):
        one_dirs = _dirs(sv, [[row[r]] for row in sets])
        _fill(sv, 1, float("nan"))
        one = _host(sv.tangent_data(one_dirs, 1))
        for key in OUT:
            assert _same(one[key][:, 0], three[key][:, r]), (key, r)
        for x, y in zip(sv.matrix_directions(one_dirs, 1), rows3):
            assert _same(x.cpu().numpy()[:, 0], y[:, r]), r
    # problems 1, 2 of 4: everything else keeps the NaN prefill
    _fill(sv, 3, float("nan"))
    sv.tangent_data(dirs, 3, p0=1, count=2)
    sv.matrix_directions(dirs, 3, p0=1, count=2)
    bufs = dict(sv.set_buffers(3), **sv.direction_buffers(3))
    for key, x in bufs.items():
        h = x.cpu().numpy()
        assert np.isnan(h[[0, 3]]).all(), key
        if key in OUT:
            assert _same(h[1:3, :, :three[key].shape[-1]], three[key][1:3]), key
    for x, y in zip(sv.direction_buffers(3).values(), rows3):
        assert _same(x.cpu().numpy()[1:3], y[1:3])


def test_single_matrices_run(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    for only in ("A", "C"):
        dirs = _dirs(sv, [[_direction(refs, case, s, keys=(only,))] for s in seeds], (only,))
        _fill(sv, 1, float("nan"))
        got = _host(sv.tangent_data(dirs, 1))
        parts = _core_dense(sv, Ps, dirs, 1)
        for p in range(len(Ps)):
            for key in OUT:
                assert np.isfinite(got[key][p]).all() and _same(got[key][p, 0], parts[p][0][key]), (only, p, key)
        assert np.abs(got["x"]).max() > 1e-6, only


# -------------------------------------------------------------------------------- 3: the call writes no input
def test_inputs_and_workspace_are_not_written(refs):
    case = "V"
    seeds = refs.usable(case)[:4]
    sv, Ps = _solved(refs, case, seeds)
    dirs = _dirs(sv, [[_direction(refs, case, s)] for s in seeds])
    inputs = [sv.ws, sv.BAbt, sv.RSQrq, sv.DCt, sv.d, sv.ux, sv.pi, sv.lam, sv.t] + [dirs[k] for k in KEYS]
    before = [x.cpu().numpy().copy() for x in inputs]
    sv.tangent_data(dirs, 1)
    sv.matrix_directions(dirs, 1)
    sv.torch.cuda.synchronize()
    for x, want in zip(inputs, before):
        assert _same(x.cpu().numpy(), want)


# ------------------------------------------------------------------------ 4: pairing with the existing adjoint
def test_pairing_with_adjoint_data(refs):
    """|<g, tangent_data(dtheta)> - <adjoint_data(g), dtheta>| within: the tangent's gate x sum |g| max(1, |dz_ref|),
    plus the gradients' gates x sum |dtheta| max(1, |G_ref|), plus the reference's own pairing defect |<g, dz_ref> -
    <G_ref, dtheta>| -- all from the CPU oracle."""
    import test_gpu_kkt_adjoint as AT

    case = "V"
    seeds = refs.usable(case)
    assert seeds == refs.mat.usable(case)
    sv, Ps = _solved(refs, case, seeds)
    full = [_direction(refs, case, s) for s in seeds]
    dirs = _dirs(sv, [[D] for D in full])
    cots = [[refs.adj.cotangent(case, s)[1]] for s in seeds]
    dz = _host(sv.tangent_data(dirs, 1))
    G = {k: v.cpu().numpy().copy() for k, v in sv.adjoint_data(AT._dense_cot(sv, cots), 1).items()}
    hdirs = {k: v.cpu().numpy() for k, v in dirs.items()}
    for p, (P, seed) in enumerate(zip(Ps, seeds)):
        g = cots[p][0]
        zref, zalt = refs.tangent(case, seed)
        mref, malt = refs.mat.gradients(case, seed)
        vref, valt = refs.adj.adjoint(case, seed)
        gref = dict(MC.flat(P, mref, sv.order), **vref)
        gates = {k: refs.mat.gate(mref, malt) for k in MAT_KEYS}
        gates.update({k: refs.adj.gate(vref, valt) for k in VEC_KEYS})
        lhs = sum(float(np.sum(g[k] * dz[k][p, 0])) for k in OUT)
        rhs = sum(float(np.sum(G[k][p, 0] * hdirs[k][p, 0])) for k in KEYS)
        ref_l = sum(float(np.sum(g[k] * zref[k])) for k in OUT)
        ref_r = sum(float(np.sum(gref[k] * hdirs[k][p, 0])) for k in KEYS)
        bound = refs.gate(zref, zalt) * sum(float(np.sum(np.abs(g[k]) * np.maximum(1.0, np.abs(zref[k])))) for k in OUT)
        bound += sum(gates[k] * float(np.sum(np.abs(hdirs[k][p, 0]) * np.maximum(1.0, np.abs(gref[k])))) for k in KEYS)
        bound += abs(ref_l - ref_r)
        print(case, seed, lhs, rhs, abs(lhs - rhs), bound, abs(ref_l - ref_r))
        assert abs(lhs) > 1e-3 and abs(lhs - rhs) <= bound, (case, seed, lhs, rhs, bound)


# -------------------------------------------------------------------------------------------------- 5: refusals
def test_refusals_write_nothing(refs):
    case = "V"
    seeds = refs.usable(case)[:3]
    sv, Ps = _solved(refs, case, seeds)
    assert sv.sizes["DCt"] > 0
    dirs = _dirs(sv, [[_direction(refs, case, s)] for s in seeds])
    _fill(sv, 1, SENTINEL, scratch=SENTINEL)
    bufs, sets, rows = sv.kkt_buffers(1), sv.set_buffers(1), sv.direction_buffers(1)
    L = ocp_lib()
    ptr = lambda x, given=True: x.data_ptr() if given else None

    def struct(keys, stride=None):
        ds = _OcpData()
        for i, key in enumerate(KEYS):
            if key in keys:
                ds.ptr[i], ds.stride[i] = dirs[key].data_ptr(), sv.sizes[key] if stride is None else stride
        return ds

    def core(ndir=1, p0=0, count=3, plan=True, keys=KEYS, ds=True, ux=True, pi=True, lam=True, b=True, q=True, d=True,
             stride=None):
        return L.hpmpc_mi355x_ocp_matrix_dirs_batch(
            sv.plan if plan else None, C.byref(struct(keys, stride)) if ds else None, sv.nprob, p0, count, ndir,
            ptr(sv.ux, ux), ptr(sv.pi, pi), ptr(sv.lam, lam), ptr(rows["db"], b), ptr(rows["dq"], q),
            ptr(rows["dd"], d), sv._stream())

    def both(ndir=1, p0=0, count=3, plan=True, keys=KEYS, ds=True, ux=True, pi=True, lam=True, scratch=True, ws=True,
             DCt=True, out=True, stride=None):
        return L.hpmpc_mi355x_ocp_tangent_data_batch(
            sv.plan if plan else None, C.byref(struct(keys, stride)) if ds else None, sv.nprob, p0, count, ndir,
            ptr(sv.BAbt), ptr(sv.RSQrq), ptr(sv.DCt, DCt), ptr(sv.ux, ux), ptr(sv.pi, pi), ptr(sv.lam, lam),
            ptr(sets["u"], out), *(ptr(sets[k]) for k in OUT[1:]), ptr(sv.ws, ws), ptr(bufs["scratch"], scratch), 1,
            sv._stream())

    calls = [core(ndir=0), core(ndir=-1), core(ndir=2 ** 30), core(p0=1, count=3), core(p0=-1, count=1),
             core(plan=False), core(ds=False), core(ux=False), core(pi=False), core(lam=False), core(b=False),
             core(q=False), core(d=False), core(keys=("Q",), stride=1), core(keys=("q",), stride=1),
             both(ndir=0), both(ndir=2 ** 30), both(p0=2, count=2), both(p0=-1, count=1), both(plan=False),
             both(ds=False), both(ux=False), both(pi=False), both(lam=False), both(scratch=False), both(ws=False),
             both(DCt=False), both(out=False), both(keys=("Q",), stride=1), both(keys=("q",), stride=1)]
    for i, rc in enumerate(calls):
        assert rc == EUNSUPPORTED, i
    assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    assert core(count=0) == 0 and both(count=0) == 0 and core(count=0, ux=False) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    for key, x in list(bufs.items()) + list(sets.items()) + list(rows.items()):
        h = x.cpu().numpy()
        assert _same(h, np.full_like(h, SENTINEL)), key
    # what is not needed may be null: no pi without A and B, no lam without C and D
    assert core(keys=("Q", "S", "R", "C", "D") + VEC_KEYS, pi=False) == 0
    assert core(keys=("A", "B", "Q") + VEC_KEYS, lam=False) == 0
    assert both(keys=("Q", "S", "R") + VEC_KEYS, pi=False, lam=False) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    assert all(np.isfinite(x.cpu().numpy()).all() for x in list(sets.values()) + list(rows.values()))
    with pytest.raises(ValueError):
        sv.tangent_data(dirs, 2)  # the tensors hold one direction per problem
    with pytest.raises(ValueError):
        sv.tangent_data({"u": dirs["r"]}, 1)
    with pytest.raises(ValueError):
        sv.matrix_directions({"A": dirs["A"][:, :, :-1]}, 1)
    with pytest.raises(RuntimeError):
        sv.tangent({"A": dirs["A"]}, 1)  # the dense tangent call keeps refusing matrix entries

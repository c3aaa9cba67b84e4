"""The batched soft KKT re-solve on the GPU: hpmpc_mi355x_soft_kkt_batch (SoftBatchSolver.kkt_new_rhs) and
hpmpc_mi355x_soft_kkt_ocp_batch (OcpSoftBatchSolver.kkt_sets / resolve) against the numpy reference of
tests/soft_kkt_cases.py on its admitted draws (tests/test_soft_kkt_host.py holds the admission rule).

Gate: TOL_SOFT of tests/helpers.py -- ux, t at 5e-8 and pi, lam at 1e-6, relative to max(1, |ref|).  The inputs are well
conditioned (Lam in [0.25, 4]); every comparison prints its worst error as a share of its gate before it asserts
(DESIGN.md §9 lists them per case).
"""
import functools

import numpy as np
import pytest

import ocp_soft_cases as OC
import soft_kkt_cases as K
from helpers import TOL_SOFT
from hpmpc_amd.bindings import lib
from hpmpc_amd.ocp_soft import (OcpSoftBatchSolver, flatten_soft_problems, flatten_soft_sets,
                                unflatten_soft_set_outputs)
from hpmpc_amd.soft import SoftBatchSolver, random_soft_qp

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
NAN = float("nan")


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def dev(a):
    import torch

    return torch.from_numpy(np.ascontiguousarray(a, dtype=np.float64)).to("cuda")


def host(x):
    return x.cpu().numpy()


@functools.lru_cache(maxsize=None)
def batch(case, seeds=None):
    """The admitted draws of a case as one batch, with the reference solution of every (problem, set): computed once,
    shared by the tests and left unchanged."""
    draws = [K.draw(case, s) for s in (K.admitted(case) if seeds is None else seeds)]
    refs = [[K.newton_reference(P, [l / t for l, t in zip(lam, tt)], tt, S) for S in sets]
            for P, lam, tt, sets in draws]
    return draws, refs


def packed_inputs(draws, nrhs):
    cols = [K.padded_sets(P, sets[:nrhs]) for P, _, _, sets in draws]
    b, q, d, z = (dev(np.stack([c[i] for c in cols])) for i in range(4))
    lam0 = dev(np.stack([K.packed_iterate(P, lam) for P, lam, _, _ in draws]))
    t0 = dev(np.stack([K.packed_iterate(P, t) for P, _, t, _ in draws]))
    return b, q, d, z, lam0, t0


def soft_solver(draws, **kw):
    return SoftBatchSolver(K.soft_qps([d[0] for d in draws]), k_max=OC.ARGS["k_max"], **kw)


def ocp_solver(draws, order="C", z=True):
    """z=False: the front end gets no z and packs zeros, as for the admitted solves of ocp_soft_cases.DRAWS."""
    Ps = [d[0] for d in draws]
    P = Ps[0]
    data = {k: dev(v) for k, v in flatten_soft_problems(Ps, order).items() if z or k != "z"}
    sv = OcpSoftBatchSolver(P["N"], P["nx"], P["nu"], P["nb"], P["hidxb"], P["ns"], data, nprob=len(Ps), order=order,
                            k_max=OC.ARGS["k_max"])
    sv.pack()
    return sv


def dense_sets(draws, nrhs):
    return {k: dev(v) for k, v in flatten_soft_sets([[K.with_set(P, S) for S in sets[:nrhs]]
                                                     for P, _, _, sets in draws]).items()}


def worst_share(draws, refs, got, nrhs, label):
    """got(p, r) -> per-stage lists; prints and returns the worst error per vector as a share of its gate."""
    worst = dict(ux=0.0, pi=0.0, lam=0.0, t=0.0)
    for p, (P, _, _, _) in enumerate(draws):
        for r in range(nrhs):
            e = K.gate_share(K.rel_errors(P, got(p, r), refs[p][r]))
            worst = {k: max(worst[k], e[k]) for k in worst}
    print(f"{label}: worst error as a share of its gate " + ", ".join(f"{k} {v:.2e}" for k, v in worst.items()))
    return worst


def padded_getter(draws, out):
    ux, pi, lam, t = (host(x) for x in out)
    return lambda p, r: K.unpack_padded(draws[p][0], ux[p, r], pi[p, r], lam[p, r], t[p, r])


def dense_getter(draws, out):
    P0 = draws[0][0]
    per = unflatten_soft_set_outputs({k: host(v) for k, v in out.items()}, P0["N"], P0["nx"], P0["nu"], P0["nb"],
                                     P0["ns"])

    def get(p, r):
        P, o = draws[p][0], per[p][r]
        return dict(ux=[np.r_[o["u"][k] if k < P["N"] else np.zeros(0), o["x"][k]] for k in range(P["N"] + 1)],
                    pi=o["pi"], lam=K.compact_to_padded(P, o["lam"]), t=K.compact_to_padded(P, o["t"]))
    return get


def set_iterate(sv, lam0, t0):
    sv.lam[:, :lam0.shape[1]].copy_(lam0)
    sv.t[:, :t0.shape[1]].copy_(t0)


# ---- 1. refactor = 1 at a given (lam, t) ----

@pytest.mark.parametrize("nrhs", (1, 3))
@pytest.mark.parametrize("case", K.CASES)
def test_refactor_packed(case, nrhs):
    draws, refs = batch(case)
    sv = soft_solver(draws)
    b, q, d, z, lam0, t0 = packed_inputs(draws, nrhs)
    sv.ws.fill_(NAN)  # the factor launch needs no initialised workspace
    out = sv.kkt_new_rhs(b, q, d, z, nrhs=nrhs, refactor=True, lam0=lam0, t0=t0)
    sv.torch.cuda.synchronize()
    w = worst_share(draws, refs, padded_getter(draws, out), nrhs, f"{case} packed nrhs {nrhs}")
    assert max(w.values()) <= 1.0, w


@pytest.mark.parametrize("order", ("C", "F"))
@pytest.mark.parametrize("nrhs", (1, 3))
@pytest.mark.parametrize("case", K.CASES)
def test_refactor_ocp(case, nrhs, order):
    draws, refs = batch(case)
    sv = ocp_solver(draws, order)
    _, _, _, _, lam0, t0 = packed_inputs(draws, nrhs)
    set_iterate(sv, lam0, t0)
    out = sv.kkt_sets(dense_sets(draws, nrhs), nrhs, refactor=True)
    sv.torch.cuda.synchronize()
    w = worst_share(draws, refs, dense_getter(draws, out), nrhs, f"{case} ocp {order} nrhs {nrhs}")
    assert max(w.values()) <= 1.0, w


# ---- 2. refactor = 0 after a solve ----

def test_persisted_linearisation():
    draws, _ = batch("D", tuple(OC.seeds("D")))
    assert min(OC.kks("D")) >= 9
    a = OC.args_of("D")
    opts = dict(mu0=a["mu0"], mu_tol=a["mu_tol"], alpha_min=a["alpha_min"])
    nrhs = 2
    sets = dense_sets(draws, nrhs)
    sv = ocp_solver(draws, z=False)
    sv.solve(k_max=4, **opts)
    sv.torch.cuda.synchronize()
    assert host(sv.kk).tolist() == [4] * len(draws)
    ws0 = host(sv.ws).copy()
    got = {k: v.clone() for k, v in sv.kkt_sets(sets, nrhs, refactor=False).items()}
    sv.torch.cuda.synchronize()
    assert _same(ws0, host(sv.ws)), "refactor = 0 only reads ws"
    # the iterate the fourth iteration linearised at: a second solver stopped after three
    s3 = ocp_solver(draws, z=False)
    s3.solve(k_max=3, **opts)
    s3.torch.cuda.synchronize()
    assert host(s3.kk).tolist() == [3] * len(draws)
    lam3, t3 = host(s3.lam), host(s3.t)
    lay = K.soft_batch_layout(OC.soft_qp(draws[0][0], True))
    refs = []
    for p, (P, _, _, ss) in enumerate(draws):
        n = lambda k: 2 * K.sizes(P, k)[4] + 4 * K.sizes(P, k)[5]
        cut = lambda v: [v[p, int(lay["oC"][k]):int(lay["oC"][k]) + n(k)].copy() for k in range(P["N"] + 1)]
        lam, t = cut(lam3), cut(t3)
        for k in range(P["N"] + 1):  # padding: lam 0, t 1, so Lam is finite there
            pad = np.setdiff1d(np.arange(len(t[k])), K.live_slots(P, k))
            t[k][pad], lam[k][pad] = 1.0, 0.0
        refs.append([K.newton_reference(P, [l / tt for l, tt in zip(lam, t)], t, S) for S in ss[:nrhs]])
    w = worst_share(draws, refs, dense_getter(draws, got), nrhs, "D refactor 0 against the numpy reference at iterate 3")
    assert max(w.values()) <= 1.0, w
    own = s3.kkt_sets(sets, nrhs, refactor=True)
    s3.torch.cuda.synchronize()
    worst = 0.0
    for key, gate in (("u", "ux"), ("x", "ux"), ("pi", "pi"), ("lam", "lam"), ("t", "t")):
        g, r = host(got[key]), host(own[key])
        e = float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)), initial=0.0)) / TOL_SOFT[gate]
        print(f"D refactor 0 against refactor 1 at iterate 3: {key} {e:.2e} of its gate")
        worst = max(worst, e)
    assert worst <= 1.0


# ---- 3. affinity ----

def test_affine_in_the_set():
    draws, _ = batch("odd")
    draws = [(P, lam, t, [S[0], S[1], None]) for P, lam, t, S in draws]
    for P, lam, t, S in draws:  # v, v + delta, v + 2 delta
        S[2] = {k: [2.0 * np.asarray(b) - np.asarray(a) for a, b in zip(S[0][k], S[1][k])] for k in K.SET_KEYS}
    sv = soft_solver(draws)
    b, q, d, z, lam0, t0 = packed_inputs(draws, 3)
    out = sv.kkt_new_rhs(b, q, d, z, nrhs=3, refactor=True, lam0=lam0, t0=t0)
    sv.torch.cuda.synchronize()
    for name, x in zip(("ux", "pi", "lam", "t"), out):
        x = host(x)
        dd = np.abs(x[:, 0] - 2.0 * x[:, 1] + x[:, 2]) / np.maximum(1.0, np.abs(x[:, 1]))
        print(f"second difference of {name}: {dd.max():.2e}")
        assert dd.max() <= 1e-10, name


# ---- 4. range and isolation ----

def test_range_and_isolation():
    draws, refs = batch("stray")
    draws, refs = draws[:4], refs[:4]
    sv = soft_solver(draws)
    nrhs = 2
    b, q, d, z, lam0, t0 = packed_inputs(draws, nrhs)
    set_iterate(sv, lam0, t0)
    sv.ux.fill_(0.25)
    sv.pi.fill_(-0.5)
    keep = dict(BAbt=sv.BAbt, RSQrq=sv.RSQrq, Z=sv.Z, d0=sv.d, z0=sv.z, ux=sv.ux, pi=sv.pi, lam=sv.lam, t=sv.t, b=b, q=q,
                d=d, z=z)
    before = {k: host(v).copy() for k, v in keep.items()}
    out = sv.kkt_buffers(nrhs)
    for k in ("ux", "pi", "lam", "t"):
        out[k].fill_(NAN)
    sv.kkt_new_rhs(b, q, d, z, nrhs=nrhs, refactor=True, p0=1, count=2)
    sv.torch.cuda.synchronize()
    for k in ("ux", "pi", "lam", "t"):
        x = host(out[k])
        assert np.isnan(x[0]).all() and np.isnan(x[3]).all(), k
    get = padded_getter(draws, tuple(out[k] for k in ("ux", "pi", "lam", "t")))
    for p in (1, 2):
        for r in range(nrhs):
            e = K.gate_share(K.rel_errors(draws[p][0], get(p, r), refs[p][r]))
            assert max(e.values()) <= 1.0, (p, r, e)
    sv.kkt_new_rhs(b, q, d, None, nrhs=nrhs, refactor=False, p0=0, count=1)
    sv.torch.cuda.synchronize()
    for k, v in keep.items():
        assert _same(before[k], host(v)), k


# ---- 5. shared layout ----

def test_shared_layout_is_bitwise_the_unshared():
    # one problem's matrices in every problem of the batch; the sets and the base iterates still differ
    draws, _ = batch("D")
    P0 = draws[0][0]
    draws = [(dict(P0), lam, t, sets) for _, lam, t, sets in draws[:4]]
    nrhs = 3
    b, q, d, z, lam0, t0 = packed_inputs(draws, nrhs)
    outs = []
    for shared in (False, True):
        sv = soft_solver(draws, shared=shared)
        o = sv.kkt_new_rhs(b, q, d, z, nrhs=nrhs, refactor=True, lam0=lam0, t0=t0)
        sv.torch.cuda.synchronize()
        outs.append([host(x).copy() for x in o])
    assert np.abs(outs[0][0]).max() > 0
    for a, bb, name in zip(outs[0], outs[1], ("ux", "pi", "lam", "t")):
        assert _same(a, bb), name


# ---- 6. z null ----

def test_null_z_is_the_problems_z():
    draws, _ = batch("Q")
    nrhs = 3
    sv = soft_solver(draws)
    b, q, d, _, lam0, t0 = packed_inputs(draws, nrhs)
    zrep = sv.z[:, None, :].expand(-1, nrhs, -1).contiguous()
    outs = []
    for z in (zrep, None):
        o = sv.kkt_new_rhs(b, q, d, z, nrhs=nrhs, refactor=True, lam0=lam0, t0=t0)
        sv.torch.cuda.synchronize()
        outs.append([host(x).copy() for x in o])
    assert np.abs(outs[0][2]).max() > 0
    for a, bb, name in zip(outs[0], outs[1], ("ux", "pi", "lam", "t")):
        assert _same(a, bb), name


# ---- 7. refusals ----

def test_refusals_write_nothing():
    import ctypes as C

    draws, _ = batch("N1")
    sv = soft_solver(draws)
    nrhs, P = 1, len(draws)
    b, q, d, z, lam0, t0 = packed_inputs(draws, nrhs)
    out = sv.kkt_buffers(nrhs)
    sv.ws.fill_(0.5)
    for k in ("ux", "pi", "lam", "t", "scratch"):
        out[k].fill_(NAN)
    watch = dict(out, ws=sv.ws)
    before = {k: host(v).copy() for k, v in watch.items()}
    L = lib()
    ptr = lambda x: None if x is None else x.data_ptr()

    def call(plan=None, nrhs=1, p0=0, count=P, b=b, lam0=lam0, refactor=1):
        return L.hpmpc_mi355x_soft_kkt_batch(
            sv.plan if plan is None else plan, C.byref(sv.layout), P, p0, count, nrhs, ptr(sv.BAbt), ptr(sv.RSQrq),
            ptr(sv.Z), ptr(sv.z), ptr(lam0), ptr(t0), ptr(b), ptr(q), ptr(d), ptr(z), ptr(out["ux"]), ptr(out["pi"]),
            ptr(out["lam"]), ptr(out["t"]), ptr(sv.ws), ptr(out["scratch"]), refactor, 1, sv._stream())

    assert call(nrhs=0) == EUNSUPPORTED
    assert call(b=None) == EUNSUPPORTED
    assert call(lam0=None, refactor=1) == EUNSUPPORTED
    assert call(p0=1, count=P) == EUNSUPPORTED and call(p0=-1, count=1) == EUNSUPPORTED
    assert call(count=0) == 0
    # a plan with no constraint on any stage: the sizes of N1 without its boxes
    free = random_soft_qp(1, [0, 3], [2, 0], [0, 0], [0, 0], seed=0)
    fs = SoftBatchSolver([free] * P, k_max=4)
    assert call(plan=fs.plan) == EUNSUPPORTED
    sv.torch.cuda.synchronize()
    for k, v in watch.items():
        assert _same(before[k], host(v)), k


# ---- 8. resolve ----

def test_resolve_is_one_set_and_leaves_the_solve_alone():
    draws, _ = batch("D", tuple(OC.seeds("D")))
    a = OC.args_of("D")
    sv = ocp_solver(draws, z=False)
    sv.solve(mu0=a["mu0"], mu_tol=a["mu_tol"], alpha_min=a["alpha_min"])
    first = {k: host(v).copy() for k, v in sv.finish().items()}
    packed = {k: host(v).copy() for k, v in dict(BAbt=sv.BAbt, RSQrq=sv.RSQrq, d=sv.d, Z=sv.Zp, z=sv.zp).items()}
    sets = dense_sets(draws, 1)
    want = {k: host(v).copy() for k, v in sv.kkt_sets(sets, 1, refactor=True).items()}
    for v in sv.kkt_buffers(1).values():
        v.fill_(NAN)
    got = sv.resolve({k: v[:, 0].contiguous() for k, v in sets.items()}, refactor=True)
    sv.torch.cuda.synchronize()
    assert set(got) == set(first) - {"kk", "status", "inf_norm_res"}
    for k in got:
        assert np.isfinite(want[k]).all() and _same(want[k][:, 0], host(got[k])), k
    again = {k: host(v) for k, v in sv.finish().items()}
    for k in first:
        assert _same(first[k], again[k]), k
    for k, v in dict(BAbt=sv.BAbt, RSQrq=sv.RSQrq, d=sv.d, Z=sv.Zp, z=sv.zp).items():
        assert _same(packed[k], host(v)), k

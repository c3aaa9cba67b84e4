"""The batched KKT re-solve (hpmpc_mi355x_kkt_new_rhs_batch, hpmpc_mi355x_ocp_kkt_batch, hk_kkt.hip; Python:
BatchSolver.kkt_new_rhs, OcpBatchSolver.resolve / kkt_sets) on the GPU against the CPU oracle's
d_kkt_solve_new_rhs_res_mpc_hard_tv.

Inputs: the cases V, V0, F, S, H, E, B of ocp_batch_cases with seeds 0..9.  The "tightened" problems have lb, ub, lg,
ug multiplied by 0.25 and are solved with mu0 = 2, mu_tol = 1e-4, alpha_min = 1e-8, k_max = 50: the untightened
random problems end with every |lam| < 1e-5, which would leave the constraint half of the re-solve untested, and at
mu_tol = 1e-10 the 1/t terms of the last Newton system spread the oracle's own two builds by up to 4e-4.  Every test
on tightened problems asserts its preconditions (`usable`): only problems with oracle status != 0 are left out and
at most 1 of 10 per case; the two oracle builds (liboracle.so, liboracle_fma.so) agree on kk and their re-solves
differ by at most TOL_IPM / 4 on every problem and right-hand side used; at least 8 of 10 problems (S: 5 of 10) end
with a multiplier above 1e-2.  Gates: TOL_IPM = 1e-10 relative to max(1, |ref|), inf_norm_res 1e-9 absolute; the
untightened test uses the GATES rule max(TOL_IPM, 4 x the spread of the oracle's builds).
"""
import os

import numpy as np
import pytest

from helpers import TOL_IPM
from hpmpc_amd.cabi import bq_from_qp
from hpmpc_amd.ocp_batch import flatten_problems, kkt_set_arrays, ocp_lib
from ocp_batch_cases import IO, K_MAX, check, compact, make_solver, pack_problems, problems, to_device

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
SENTINEL = -7.25
SEEDS = range(10)
TIGHT = dict(mu0=2.0, mu_tol=1e-4, alpha_min=1e-8)
LOOSE = dict(mu0=2.0, mu_tol=1e-10, alpha_min=1e-8)
# problems (of 10) that must end with a multiplier above 1e-2
MIN_ACTIVE = {"V": 8, "V0": 8, "F": 8, "S": 5, "H": 8, "E": 8, "B": 8}


def fma_oracle():
    """The oracle compiled with -mfma -ffp-contract=fast: the second build of the spread (test_gpu_general.py)."""
    from hpmpc_amd.cabi import HpmpcAPI, load

    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    return HpmpcAPI(load(os.path.join(root, "oracle", "liboracle_fma.so")), "orc_")


def tighten(P):
    """P with lb, ub, lg, ug multiplied by 0.25 (the bounds become active at the solution)."""
    Q = dict(P)
    for key in ("lb", "ub", "lg", "ug"):
        Q[key] = [0.25 * np.asarray(v) for v in P[key]]
    return Q


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


def _rel(a, b):
    a, b = np.asarray(a), np.asarray(b)
    return float(np.max(np.abs(a - b) / np.maximum(1.0, np.abs(b)), initial=0.0))


def _sized(P, r):
    """An iterate's real entries, per stage: ux (nu + nx), pi (nx[k+1]), lam and t compact."""
    N = P["N"]
    return dict(ux=[np.asarray(r["ux"][k])[:P["nu"][k] + P["nx"][k]] for k in range(N + 1)],
                pi=[np.asarray(r["pi"][k])[:P["nx"][k + 1]] for k in range(N)],
                lam=compact(P, r["lam"]), t=compact(P, r["t"]))


def _iter_err(P, got, ref):
    g, r = _sized(P, got), _sized(P, ref)
    return max(_rel(a, b) for key in g for a, b in zip(g[key], r[key]))


class Refs:
    """Oracle solves and re-solves, computed once per key and shared between the tests (never modified)."""

    def __init__(self, oracle):
        self.apis = (oracle, fma_oracle())
        self.cache = {}

    def problem(self, case, seed, tight):
        P = problems(case, [seed])[0]
        return tighten(P) if tight else P

    def ipm(self, case, seed, tight):
        """(P, the IPM result of liboracle.so, of liboracle_fma.so)"""
        key = ("ipm", case, seed, tight)
        if key not in self.cache:
            P = self.problem(case, seed, tight)
            args = TIGHT if tight else LOOSE
            self.cache[key] = (P,) + tuple(api.ipm(IO.to_qp(P), k_max=K_MAX, **args) for api in self.apis)
        return self.cache[key]

    def kkt(self, case, seed, tight, rseed):
        """(P2, the re-solve of liboracle.so, of liboracle_fma.so) for the right-hand sides IO.new_rhs(P, rseed)"""
        key = ("kkt", case, seed, tight, rseed)
        if key not in self.cache:
            P, *ipms = self.ipm(case, seed, tight)
            P2 = IO.new_rhs(P, seed=rseed)
            qp2 = IO.to_qp(P2)
            b2, q2 = bq_from_qp(qp2)
            self.cache[key] = (P2,) + tuple(api.kkt_new_rhs(qp2.copy(), r["work"], b2, q2)
                                            for api, r in zip(self.apis, ipms))
        return self.cache[key]

    def usable(self, case, rseeds=(6,)):
        """The seeds of the tightened case a test may use, with the conditions every such test asserts."""
        used, active = [], 0
        for seed in SEEDS:
            P, r, rf = self.ipm(case, seed, True)
            if r["ret"] != 0:
                continue  # the only reason to leave a problem out
            assert rf["kk"] == r["kk"] and rf["ret"] == 0, (case, seed)
            for rs in rseeds:
                P2, k, kf = self.kkt(case, seed, True, rs)
                spread = _iter_err(P2, kf, k)
                assert spread <= TOL_IPM / 4, (case, seed, rs, spread)
            active += max(float(np.max(v, initial=0.0)) for v in compact(P, r["lam"])) > 1e-2
            used.append(seed)
        assert len(used) >= len(SEEDS) - 1, (case, used)
        assert active >= MIN_ACTIVE[case], (case, active)
        return used


@pytest.fixture(scope="module")
def refs(oracle):
    return Refs(oracle)


def _solved(refs, case, seeds, order, tight=True):
    """pack -> ocp_ipm_batch on the problems; kk / ret equal the oracle's."""
    ipms = [refs.ipm(case, s, tight) for s in seeds]
    Ps = [i[0] for i in ipms]
    sv = make_solver(Ps, order)
    pack_problems(sv, Ps)
    sv.solve(**(TIGHT if tight else LOOSE))
    sv.torch.cuda.synchronize()
    assert sv.kk.tolist() == [i[1]["kk"] for i in ipms], case
    assert sv.ret.tolist() == [i[1]["ret"] for i in ipms], case
    assert min(sv.kk.tolist()) >= 1
    return sv, Ps, ipms


def _dev(sv, x):
    return sv.torch.from_numpy(np.ascontiguousarray(x)).to(sv.dev)


def _set_inputs(sv, P2, nrhs):
    """P2[p][r] -> device b, q, d of shape (nprob, nrhs, N+1, .)"""
    b, q, d = kkt_set_arrays([P for row in P2 for P in row])
    shp = lambda x: _dev(sv, x.reshape((len(P2), nrhs) + x.shape[1:]))
    return shp(b), shp(q), shp(d)


def _host_sets(out):
    return [x.cpu().numpy().copy() for x in out]


def _as_iterate(h, p, r):
    return dict(ux=h[0][p, r], pi=h[1][p, r], lam=h[2][p, r], t=h[3][p, r])


# ------------------------------------------------------------------------------------------ 1: the OCP route
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", ["V", "V0", "F", "S", "H", "E", "B"])
def test_ocp_resolve_matches_the_wrapper(refs, oracle, case, order):
    seeds = refs.usable(case)
    sv, Ps, ipms = _solved(refs, case, seeds, order)
    P2s = [refs.kkt(case, s, True, 6)[0] for s in seeds]
    sv.resolve(to_device(sv, flatten_problems(P2s, order)))
    got = sv.results()
    worst = 0.0
    for p, (P, P2, g) in enumerate(zip(Ps, P2s, got)):
        ref = IO.kkt_ocp(oracle, P, P2, k_max=K_MAX, mu0=TIGHT["mu0"], mu_tol=TIGHT["mu_tol"])
        ref.update(status=ipms[p][1]["ret"], kk=ipms[p][1]["kk"])  # the IPM's: the re-solve has none of its own
        worst = max(worst, check(g, ref, keys=("u", "x", "pi", "lam"), tag=(case, order, seeds[p])))
    print(case, order, "worst relative error of the re-solve", worst)


# ------------------------------------------------------------------------ 2: untightened, mu_tol = 1e-10
@pytest.mark.parametrize("case", ["V", "F", "H", "E"])
def test_ocp_resolve_untightened(refs, case):
    seeds = [s for s in SEEDS if refs.ipm(case, s, False)[1]["ret"] == 0]
    assert len(seeds) >= len(SEEDS) - 1
    sv, Ps, ipms = _solved(refs, case, seeds, "C", tight=False)
    P2s = [IO.new_rhs(P, seed=6) for P in Ps]
    sv.resolve(to_device(sv, flatten_problems(P2s, "C")))
    got = sv.results()
    for p, (P, P2, g) in enumerate(zip(Ps, P2s, got)):
        assert ipms[p][2]["kk"] == ipms[p][1]["kk"]
        ref, alt = (IO.kkt_ocp(api, P, P2, k_max=K_MAX, mu0=LOOSE["mu0"], mu_tol=LOOSE["mu_tol"]) for api in refs.apis)
        for key in ("u", "x", "pi", "lam"):
            spread = max(_rel(a, r) for a, r in zip(alt[key], ref[key]))
            gate = max(TOL_IPM, 4 * spread)  # the GATES rule
            err = max(_rel(a, r) for a, r in zip(g[key], ref[key]))
            assert err <= gate, (case, seeds[p], key, err, gate)
        np.testing.assert_allclose(g["inf_norm_res"], ref["inf_norm_res"], rtol=0, atol=1e-9)


# ------------------------------------------------------------------------------------------------ 3: many sets
@pytest.mark.parametrize("case", ["V", "F", "H", "E"])
def test_many_sets_per_factor(refs, case):
    rseeds = (6, 7, 8)
    seeds = refs.usable(case, rseeds)[:5]
    sv, Ps, ipms = _solved(refs, case, seeds, "C")
    kk = [[refs.kkt(case, s, True, rs) for rs in rseeds] for s in seeds]
    P2 = [[k[0] for k in row] for row in kk]
    b, q, d = _set_inputs(sv, P2, 3)
    h3 = _host_sets(sv.kkt_sets(b, q, d, nrhs=3))
    for p in range(len(seeds)):
        for r in range(3):
            err = _iter_err(P2[p][r], _as_iterate(h3, p, r), kk[p][r][1])
            assert err <= TOL_IPM, (case, seeds[p], rseeds[r], err)
    for r in range(3):
        one = lambda x: x[:, r:r + 1].contiguous()
        # the same set alone in a launch
        h1 = _host_sets(sv.kkt_sets(one(b), one(q), one(d), nrhs=1))
        for a, x in zip(h1, h3):
            assert np.array_equal(_bits(a[:, 0]), _bits(x[:, r])), (case, r)
        # and with b, q read from the rows a vectors-only pack of that set wrote
        sv.pack(to_device(sv, flatten_problems([row[r] for row in P2], "C")), matrices=False)
        h0 = _host_sets(sv.kkt_sets(None, None, one(d), nrhs=1))
        for a, x in zip(h0, h3):
            assert np.array_equal(_bits(a[:, 0]), _bits(x[:, r])), (case, r)


# ----------------------------------------------------------------------------------- 4: nothing else is written
def test_only_the_sets_in_range_are_written(refs):
    case, rseeds = "V", (6, 7)
    seeds = refs.usable(case, rseeds)[:5]
    sv, Ps, ipms = _solved(refs, case, seeds, "C")
    P2 = [[refs.kkt(case, s, True, rs)[0] for rs in rseeds] for s in seeds]
    b, q, d = _set_inputs(sv, P2, 2)
    bufs = sv.kkt_buffers(2)
    names = ("ux", "pi", "lam", "t", "scratch")
    inputs = (sv.ws, sv.BAbt, sv.RSQrq, sv.DCt, d, b, q)
    before = [x.cpu().numpy().copy() for x in inputs]

    def run(fill):
        for n in names:
            bufs[n].fill_(SENTINEL)
        if fill is not None:
            bufs["scratch"][1:3].fill_(fill)
        sv.kkt_sets(b, q, d, nrhs=2, p0=1, count=2)
        sv.torch.cuda.synchronize()
        return {n: bufs[n].cpu().numpy().copy() for n in names}

    first = run(None)
    for x, want in zip(inputs, before):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(want))
    for n in names:  # the sets of problems 0, 3, 4 keep the sentinel
        for p in (0, 3, 4):
            assert np.array_equal(_bits(first[n][p]), _bits(np.full_like(first[n][p], SENTINEL))), (n, p)
    for p in (1, 2):
        for r in range(2):
            ref = refs.kkt(case, seeds[p], True, rseeds[r])[1]
            got = {n: first[n][p, r] for n in names[:4]}
            assert _iter_err(P2[p][r], got, ref) <= TOL_IPM
    # the result does not depend on what the scratch held: the same call on NaN and on the previous call's leftovers
    again = run(float("nan"))
    sv.kkt_sets(b, q, d, nrhs=2, p0=1, count=2)
    sv.torch.cuda.synchronize()
    for n in names[:4]:
        assert np.array_equal(_bits(again[n]), _bits(first[n])), n
        assert np.array_equal(_bits(bufs[n].cpu().numpy()), _bits(first[n])), n
    # compute_mult = 0: pi is not solved for and comes back as the workspace's backup (the 9th of the 16-double
    # vectors behind the factor's 352 doubles per stage), whatever the scratch held; ux, lam, t as before
    bufs["scratch"].fill_(float("nan"))
    sv.kkt_sets(b, q, d, nrhs=2, p0=1, count=2, compute_mult=0)
    sv.torch.cuda.synchronize()
    n1 = sv.N + 1
    ws = sv.ws.cpu().numpy()
    for n in ("ux", "lam", "t"):
        assert np.array_equal(_bits(bufs[n].cpu().numpy()), _bits(first[n])), n
    pi = bufs["pi"].cpu().numpy()
    for p in (1, 2):
        bkp = ws[p, n1 * 352 + 8 * n1 * 16:n1 * 352 + 9 * n1 * 16].reshape(n1, 16)
        for r in range(2):
            assert np.array_equal(_bits(pi[p, r]), _bits(bkp)), (p, r)
    for x, want in zip(inputs, before):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(want))


# ---------------------------------------------------------------------------------- 5: the plain batched route
def _batched_qp(Ps):
    from hpmpc_amd.ocp import OCPQP

    qps = [IO.to_qp(P) for P in Ps]
    q0 = qps[0]
    st = lambda key, n: [np.stack([getattr(q, key)[k] for q in qps]) for k in range(n)]
    return OCPQP(q0.N, q0.nx, q0.nu, q0.nb, q0.ng, q0.idxb, st("BAbt", q0.N), st("RSQrq", q0.N + 1),
                 st("d", q0.N + 1), [], len(qps))


def test_batch_solver_route(refs):
    from hpmpc_amd.batch import BatchSolver, kkt_lib, kkt_scratch_doubles

    case, rseeds = "V0", (6, 7)
    seeds = refs.usable(case, rseeds)
    ipms = [refs.ipm(case, s, True) for s in seeds]
    s = BatchSolver(_batched_qp([i[0] for i in ipms]), k_max=K_MAX)
    assert kkt_lib().hpmpc_mi355x_kkt_scratch_doubles(s.plan) == kkt_scratch_doubles(s.N)
    P2 = [[refs.kkt(case, sd, True, rs)[0] for rs in rseeds] for sd in seeds]
    b, q, d = _set_inputs(s, P2, 2)
    for solve in (s.ipm, s.ipm_solo):  # the four-wave solo kernel agrees to rounding: the same gate
        s.ws.zero_()
        solve(**TIGHT)
        s.torch.cuda.synchronize()
        assert s.kk.tolist() == [i[1]["kk"] for i in ipms] and s.ret.tolist() == [i[1]["ret"] for i in ipms]
        h = _host_sets(s.kkt_new_rhs(b, q, d, nrhs=2))
        assert h[0].shape == (len(seeds), 2, s.N + 1, 16) and h[2].shape == (len(seeds), 2, s.N + 1, 32)
        for p, sd in enumerate(seeds):
            for r, rs in enumerate(rseeds):
                err = _iter_err(P2[p][r], _as_iterate(h, p, r), refs.kkt(case, sd, True, rs)[1])
                assert err <= TOL_IPM, (solve.__name__, sd, rs, err)


# -------------------------------------------------------------------------------------------------- 6: refusals
def test_refusals_and_the_empty_call(refs):
    case = "V"
    seeds = refs.usable(case)[:3]
    sv, Ps, ipms = _solved(refs, case, seeds, "C")
    assert sv.sizes["DCt"] > 0
    P2 = [[refs.kkt(case, s, True, 6)[0]] for s in seeds]
    b, q, d = _set_inputs(sv, P2, 1)
    bufs = sv.kkt_buffers(1)
    outs = [bufs[n] for n in ("ux", "pi", "lam", "t", "scratch")]
    for x in outs:
        x.fill_(SENTINEL)
    L = ocp_lib()
    tile = L.hpmpc_mi355x_ocp_tile_plan(sv.plan)

    def core(nrhs=1, p0=0, count=3, DCt=True, scratch=True):
        return L.hpmpc_mi355x_kkt_new_rhs_batch(
            tile, None, sv.nprob, p0, count, nrhs, sv.BAbt.data_ptr(), sv.RSQrq.data_ptr(),
            sv.DCt.data_ptr() if DCt else None, b.data_ptr(), q.data_ptr(), d.data_ptr(), outs[0].data_ptr(),
            outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), sv.ws.data_ptr(),
            outs[4].data_ptr() if scratch else None, 1, sv._stream())

    def ocp(p0=0, count=3, scratch=True):
        return L.hpmpc_mi355x_ocp_kkt_batch(
            sv.plan, sv.nprob, p0, count, sv.BAbt.data_ptr(), sv.RSQrq.data_ptr(), sv.DCt.data_ptr(), d.data_ptr(),
            outs[0].data_ptr(), outs[1].data_ptr(), outs[2].data_ptr(), outs[3].data_ptr(), sv.ws.data_ptr(),
            outs[4].data_ptr() if scratch else None, sv._stream())

    for rc in (core(nrhs=0), core(nrhs=-1), core(scratch=False), core(DCt=False), core(p0=1, count=3),
               core(p0=-1, count=1), ocp(scratch=False), ocp(p0=2, count=2)):
        assert rc == EUNSUPPORTED
        assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    assert core(count=0) == 0 and ocp(count=0) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    for x in outs:
        h = x.cpu().numpy()
        assert np.array_equal(_bits(h), _bits(np.full_like(h, SENTINEL)))
    with pytest.raises(ValueError):
        sv.kkt_sets(b, q, d, nrhs=2)  # the arrays hold one set per problem


def test_range_and_null_refusals():
    """hpmpc_mi355x_kkt_new_rhs_batch on the smallest shape (N = 2, nx = 2, nu = 1, one box, two problems): p0 < 0,
    p0 + count > nprob (also where p0 + count or nprob * nrhs passes INT_MAX) and a null required array return
    HPMPC_MI355X_EUNSUPPORTED and leave it in hpmpc_mi355x_last_error(); count == 0 returns 0 with last_error 0;
    nothing is written."""
    Ps = problems("R", (1, 2))
    sv = make_solver(Ps, "C", k_max=5)
    L = ocp_lib()
    tile = L.hpmpc_mi355x_ocp_tile_plan(sv.plan)
    b, q, d = (sv.torch.from_numpy(x.reshape(2, 1, sv.N + 1, -1)).to(sv.dev) for x in kkt_set_arrays(Ps))
    bufs = sv.kkt_buffers(1)
    outs = [bufs[n] for n in ("ux", "pi", "lam", "t", "scratch")]
    for x in outs:
        x.fill_(SENTINEL)
    p = lambda x, given=True: x.data_ptr() if given else None

    def core(p0, count, ok=True, nrhs=1):
        return L.hpmpc_mi355x_kkt_new_rhs_batch(tile, None, sv.nprob, p0, count, nrhs, p(sv.BAbt), p(sv.RSQrq), None,
                                                p(b), p(q), p(d), p(outs[0], ok), p(outs[1]), p(outs[2]), p(outs[3]),
                                                p(sv.ws), p(outs[4]), 1, sv._stream())

    for args in ((-1, 1), (1, 2), (0, 3), (2, 1), (2 ** 31 - 1, 1), (0, 2, False), (0, 2, True, 2 ** 30)):
        assert core(*args) == EUNSUPPORTED, args
        assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED, args
    for args in ((0, 0), (2, 0), (0, 0, False)):  # an empty range asks for no array
        assert core(*args) == 0, args
        assert L.hpmpc_mi355x_last_error() == 0, args
    sv.torch.cuda.synchronize()
    for x in outs:
        assert bool((x == SENTINEL).all())

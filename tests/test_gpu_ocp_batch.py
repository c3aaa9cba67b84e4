"""The batched OCP front end (hpmpc_mi355x_ocp_*, hk_ocp.hip, hpmpc_amd/ocp_batch.py) on the GPU.

Packing is pure data movement, so it is compared bit for bit with oracle/iface_oracle.py to_qp, every lib4 block
whole (padding included) and every 32-double d slot.  Solves are compared per problem with IO.ip_ocp over the CPU
oracle at the gates of tests/test_gpu_iface.py: identical status and kk, u / x / pi / lam (and t) at TOL_IPM =
1e-10 relative to max(1, |ref|), inf_norm_res at 1e-9 absolute; every problem used has oracle status 0 (asserted).
General constraints over a batch are in tests/test_gpu_ocp_batch_general.py.
"""
import ctypes as C

import numpy as np
import pytest

from hpmpc_amd.ocp_batch import flatten_problems, ocp_dense_layout, ocp_lib, ocp_plan_create
from ocp_batch_cases import (ARGS, K_MAX, check, expected_packed, make_solver, oracle_ref, pack_problems,
                             packed_host, problems, solve_batch, to_device)

pytestmark = pytest.mark.gpu
EUNSUPPORTED = -10
SENTINEL = -7.25


def _bits(a):
    return np.ascontiguousarray(a).view(np.int64)


@pytest.fixture(scope="module")
def refs(oracle):
    """Oracle solutions, computed once per (case, seed) and shared (never modified)."""
    cache = {}

    def get(case, seed):
        if (case, seed) not in cache:
            P = problems(case, [seed])[0]
            cache[case, seed] = (P, oracle_ref(oracle, P))
        return cache[case, seed]

    return get


# ------------------------------------------------------------------------------------------------------- 1 .. 4: pack
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", ["V", "F", "H", "E", "B"])
def test_pack_is_bitwise(case, order):
    Ps = problems(case, range(70))  # 70 problems: more than any per-workgroup grouping
    sv = make_solver(Ps, order)
    for x in (sv.BAbt, sv.RSQrq, sv.DCt, sv.d):
        x.fill_(float("nan"))
    pack_problems(sv, Ps)
    got = packed_host(sv)
    for p, P in enumerate(Ps):
        for name, want in expected_packed(sv, P).items():
            assert np.array_equal(got[name][p], want), (p, name)


def test_pack_sub_range():
    Ps = problems("V", range(12))
    sv = make_solver(Ps, "C")
    for x in (sv.BAbt, sv.RSQrq, sv.DCt, sv.d, sv.ux):
        x.fill_(SENTINEL)
    sv.pack(to_device(sv, flatten_problems(Ps, "C")), p0=3, count=5)
    got = packed_host(sv)
    got["ux"] = sv.ux.cpu().numpy()
    inside = range(3, 8)
    for p, P in enumerate(Ps):
        if p in inside:
            for name, want in expected_packed(sv, P).items():
                assert np.array_equal(got[name][p], want), (p, name)
        else:
            for name in got:
                assert np.array_equal(_bits(got[name][p]), _bits(np.full_like(got[name][p], SENTINEL))), (p, name)
    assert np.array_equal(_bits(got["ux"]), _bits(np.full_like(got["ux"], SENTINEL)))  # no warm start: ux untouched


@pytest.mark.parametrize("order", ["C", "F"])
def test_pack_vectors_only(order):
    first, second = problems("V", range(6)), problems("V", range(100, 106))
    sv = make_solver(first, order)
    pack_problems(sv, first)
    before = packed_host(sv)
    pack_problems(sv, second, matrices=False)
    got = packed_host(sv)
    for p, (P1, P2) in enumerate(zip(first, second)):
        a, b = expected_packed(sv, P1), expected_packed(sv, P2)
        assert np.array_equal(before["BAbt"][p], a["BAbt"]) and not np.array_equal(a["RSQrq"], b["RSQrq"])
        # the vector rows (b of BAbt_k, r / q of RSQrq_k) and d are the second set's, all else bitwise the first's
        want = {k: v.copy() for k, v in a.items()}
        want["d"] = b["d"]
        for k in range(P1["N"] + 1):
            nux, nx1 = P1["nu"][k] + P1["nx"][k], (P1["nx"][k + 1] if k < P1["N"] else 0)
            row = lambda sd, j: (nux // 4) * 4 * sd + nux % 4 + 4 * j
            for j in range(nx1):
                i = sv.offsets["BAbt"][k] + row((nx1 + 1) // 2 * 2, j)
                want["BAbt"][i] = b["BAbt"][i]
            for j in range(nux):
                i = sv.offsets["RSQrq"][k] + row((nux + 1) // 2 * 2, j)
                want["RSQrq"][i] = b["RSQrq"][i]
        for name in want:
            assert np.array_equal(_bits(got[name][p]), _bits(want[name])), (p, name)
        assert not np.array_equal(got["BAbt"][p], a["BAbt"]) and not np.array_equal(got["BAbt"][p], b["BAbt"])


def test_pack_shared_arrays():
    Ps = problems("V", range(5))
    for P in Ps[1:]:  # one set of matrices for the whole batch
        for key in ("A", "B", "Q", "S", "R"):
            P[key] = Ps[0][key]
    flat = flatten_problems(Ps, "C")
    sv = make_solver(Ps, "C")
    data = to_device(sv, flat)
    for key in ("A", "B", "Q", "S", "R"):
        data[key] = data[key][0].clone()  # no batch dimension: stride 0
        assert data[key].dim() == 1
    for x in (sv.BAbt, sv.RSQrq, sv.DCt, sv.d):
        x.fill_(float("nan"))
    sv.pack(data)
    shared = packed_host(sv)
    sv.pack(to_device(sv, flat))  # the replicated data
    full = packed_host(sv)
    for name in full:
        assert np.array_equal(shared[name], full[name]), name
    for p, P in enumerate(Ps):
        for name, want in expected_packed(sv, P).items():
            assert np.array_equal(shared[name][p], want), (p, name)


# --------------------------------------------------------------------------------------------------- 5 .. 8: solves
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", ["V0", "F", "S", "H", "B"])
def test_solve_parity(refs, case, order):
    seeds = (1, 2, 3)
    Ps, ref = zip(*[refs(case, s) for s in seeds])
    assert all(r["status"] == 0 for r in ref)
    sv, got = solve_batch(list(Ps), order)
    worst = max(check(g, r, tag=(case, order, p)) for p, (g, r) in enumerate(zip(got, ref)))
    print(case, order, "worst relative error of the solve", worst)


@pytest.mark.parametrize("order", ["C", "F"])
def test_same_answer_as_the_one_problem_wrapper(product, refs, order):
    P, _ = refs("F", 2)
    one = product.ip_ocp(P, P["N"], order=order, k_max=K_MAX, mu0=ARGS["mu0"], mu_tol=ARGS["mu_tol"])
    sv, got = solve_batch([P], order)
    # the wrapper runs the four-wave kernel: to rounding, not bitwise
    check(got[0], one, keys=("u", "x", "pi", "lam"), tag=order)


def test_warm_start(oracle):
    Ps = problems("F", (4, 5))
    cold = [oracle_ref(oracle, P) for P in Ps]
    warm = [dict(u=[0.9 * v for v in c["u"]], x=[0.9 * v for v in c["x"]]) for c in cold]
    ref = [oracle_ref(oracle, P, warm=w) for P, w in zip(Ps, warm)]
    sv, got = solve_batch(Ps, "C", warm=warm)
    for p, (g, r) in enumerate(zip(got, ref)):
        check(g, r, tag=p)


def _equality_boxes(case, fixed):
    """Stage 1's input boxes `fixed` with lb == ub: finish returns lb there, and the iterate's bits everywhere else."""
    Ps = problems(case, (6, 7))
    for P in Ps:
        P["ub"][1] = P["ub"][1].copy()
        P["ub"][1][fixed] = P["lb"][1][fixed]  # inputs `fixed` of stage 1: lb == ub
    assert list(Ps[0]["hidxb"][1][fixed]) == fixed and Ps[0]["nu"][1] > max(fixed)
    sv, got = solve_batch(Ps, "F")
    ux = sv.ux.cpu().numpy().reshape(len(Ps), -1, 16)
    for p, (P, g) in enumerate(zip(Ps, got)):
        assert np.array_equal(g["u"][1][fixed], P["lb"][1][fixed])
        # every other entry is the iterate's
        for k in range(P["N"]):
            keep = [j for j in range(P["nu"][k]) if k != 1 or j not in fixed]
            assert np.array_equal(_bits(g["u"][k][keep]), _bits(ux[p, k, keep]))
            assert np.array_equal(_bits(g["x"][k]), _bits(ux[p, k, P["nu"][k]:P["nu"][k] + P["nx"][k]]))
        assert np.array_equal(_bits(g["x"][P["N"]]), _bits(ux[p, P["N"], :P["nx"][P["N"]]]))


def test_equality_box(oracle):
    _equality_boxes("F", [1])


def test_equality_box_on_every_input(oracle):
    """B's stage 1: nu = 8 with all eight inputs boxed and every one an equality, so the fix loop of the unpack runs its
    nbu = 8 times and no input of the stage is left to the iterate."""
    _equality_boxes("B", list(range(8)))


# ------------------------------------------------------------------------------------------- 9, 10: refusals, tile plan
def _ipm_args(sv, mu0, count, BAbt=True):
    return (sv.plan, sv.nprob, 0, count, sv.BAbt.data_ptr() if BAbt else None, sv.RSQrq.data_ptr(), None,
            sv.d.data_ptr(), sv.ux.data_ptr(), sv.pi.data_ptr(), sv.lam.data_ptr(), sv.t.data_ptr(), sv.ws.data_ptr(),
            sv.k_max, mu0, 1e-10, 1e-8, 0, 1, sv.kk.data_ptr(), sv.ret.data_ptr(), sv.stat.data_ptr(), sv._stream())


def test_refusals_and_the_empty_call(refs):
    L = ocp_lib()
    Ps = [refs("F", s)[0] for s in (1, 2)]
    sv = make_solver(Ps, "C")
    pack_problems(sv, Ps)
    state = (sv.BAbt, sv.RSQrq, sv.d, sv.ux, sv.pi, sv.lam, sv.t, sv.stat, sv.u, sv.x, sv.pi_out, sv.lam_out,
             sv.t_out, sv.inf_norm_res, sv.res)
    for x in state[3:]:
        x.fill_(SENTINEL)
    sv.kk.fill_(-3)
    sv.ret.fill_(-3)
    sv.torch.cuda.synchronize()
    before = [x.cpu().numpy().copy() for x in state]
    for mu0 in (0.0, -1.0):  # the wrappers' cost-based mu0 is per problem: refused here
        assert L.hpmpc_mi355x_ocp_ipm_batch(*_ipm_args(sv, mu0, sv.nprob)) == EUNSUPPORTED
        assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    assert L.hpmpc_mi355x_ocp_ipm_batch(*_ipm_args(sv, 2.0, sv.nprob, BAbt=False)) == EUNSUPPORTED
    ds = sv.data_struct(to_device(sv, flatten_problems(Ps, "C")))
    pack = lambda count, d: L.hpmpc_mi355x_ocp_pack_batch(sv.plan, C.byref(ds), 1, sv.nprob, 0, count,
                                                          sv.BAbt.data_ptr(), sv.RSQrq.data_ptr(), None, d, None, None,
                                                          None, sv._stream())
    assert pack(sv.nprob, None) == EUNSUPPORTED
    finish = lambda count, res: L.hpmpc_mi355x_ocp_finish_batch(
        sv.plan, sv.nprob, 0, count, sv.BAbt.data_ptr(), sv.RSQrq.data_ptr(), None, sv.d.data_ptr(), sv.ux.data_ptr(),
        sv.pi.data_ptr(), sv.lam.data_ptr(), sv.t.data_ptr(), res, sv.u.data_ptr(), sv.x.data_ptr(),
        sv.pi_out.data_ptr(), sv.lam_out.data_ptr(), sv.t_out.data_ptr(), sv.inf_norm_res.data_ptr(), sv._stream())
    assert finish(sv.nprob, None) == EUNSUPPORTED
    assert L.hpmpc_mi355x_ocp_ipm_batch(*_ipm_args(sv, 2.0, sv.nprob + 1)) == EUNSUPPORTED  # beyond the batch
    # count = 0: returns 0 and writes nothing
    assert pack(0, sv.d.data_ptr()) == 0
    assert L.hpmpc_mi355x_ocp_ipm_batch(*_ipm_args(sv, 2.0, 0)) == 0
    assert finish(0, sv.res.data_ptr()) == 0
    assert L.hpmpc_mi355x_last_error() == 0
    sv.torch.cuda.synchronize()
    for x, b in zip(state, before):
        assert np.array_equal(_bits(x.cpu().numpy()), _bits(b))
    assert sv.kk.tolist() == [-3, -3] and sv.ret.tolist() == [-3, -3]
    # nb > nu + nx: no plan
    P = Ps[0]
    nb = list(P["nb"])
    nb[2] = P["nu"][2] + P["nx"][2] + 1
    idxb = [np.arange(n, dtype=np.int32) for n in nb]
    plan, err, _ = ocp_plan_create(P["N"], P["nx"], P["nu"], nb, idxb, P["ng"])
    assert plan is None and err == EUNSUPPORTED
    # beyond the tile: refused where the tile plan refuses
    plan, err, _ = ocp_plan_create(2, [0, 14, 14], [4, 4], [0, 0, 0], [np.zeros(0, np.int32)] * 3, [0, 0, 0])
    assert plan is None and err == EUNSUPPORTED


def test_range_and_null_refusals_of_every_call():
    """hpmpc_mi355x_ocp_pack_batch, _ocp_ipm_batch and _ocp_finish_batch each: p0 < 0, p0 + count > nprob (also where
    p0 + count passes INT_MAX) and a null required array return HPMPC_MI355X_EUNSUPPORTED and leave it in
    hpmpc_mi355x_last_error(); count == 0 returns 0 with last_error 0; none of them writes anything."""
    L = ocp_lib()
    Ps = problems("R", (1, 2))
    sv = make_solver(Ps, "C", k_max=5)
    state = (sv.BAbt, sv.RSQrq, sv.d, sv.ux, sv.pi, sv.lam, sv.t, sv.ws, sv.stat, sv.u, sv.x, sv.pi_out, sv.lam_out,
             sv.t_out, sv.inf_norm_res, sv.res)
    for x in state:
        x.fill_(SENTINEL)
    sv.kk.fill_(-3)
    sv.ret.fill_(-3)
    sv.torch.cuda.synchronize()
    ds = sv.data_struct(to_device(sv, flatten_problems(Ps, "C")))
    p = lambda x, given=True: x.data_ptr() if given else None

    def pack(p0, count, ok=True):
        return L.hpmpc_mi355x_ocp_pack_batch(sv.plan, C.byref(ds), 1, sv.nprob, p0, count, p(sv.BAbt), p(sv.RSQrq, ok),
                                             None, p(sv.d), None, None, None, sv._stream())

    def ipm(p0, count, ok=True):
        return L.hpmpc_mi355x_ocp_ipm_batch(sv.plan, sv.nprob, p0, count, p(sv.BAbt), p(sv.RSQrq), None, p(sv.d),
                                            p(sv.ux), p(sv.pi), p(sv.lam), p(sv.t), p(sv.ws, ok), sv.k_max, 2.0, 1e-10,
                                            1e-8, 0, 1, p(sv.kk), p(sv.ret), p(sv.stat), sv._stream())

    def finish(p0, count, ok=True):
        return L.hpmpc_mi355x_ocp_finish_batch(sv.plan, sv.nprob, p0, count, p(sv.BAbt), p(sv.RSQrq), None, p(sv.d),
                                               p(sv.ux), p(sv.pi), p(sv.lam), p(sv.t), p(sv.res), p(sv.u), p(sv.x),
                                               p(sv.pi_out), p(sv.lam_out), p(sv.t_out), p(sv.inf_norm_res, ok),
                                               sv._stream())

    for call in (pack, ipm, finish):
        for args in ((-1, 1), (1, 2), (0, 3), (2, 1), (2 ** 31 - 1, 1), (0, 2, False)):
            assert call(*args) == EUNSUPPORTED, (call.__name__, args)
            assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED, (call.__name__, args)
        for args in ((0, 0), (2, 0), (0, 0, False)):  # an empty range asks for no array
            assert call(*args) == 0, (call.__name__, args)
            assert L.hpmpc_mi355x_last_error() == 0, (call.__name__, args)
    sv.torch.cuda.synchronize()
    for x in state:
        assert bool((x == SENTINEL).all())
    assert sv.kk.tolist() == [-3, -3] and sv.ret.tolist() == [-3, -3]


def test_sizes_and_offsets_match_the_host_layout(refs):
    for case in ("V", "F", "H", "E", "B"):
        P = problems(case, [1])[0]
        sv = make_solver([P], "C")
        lay = ocp_dense_layout(P["N"], P["nx"], P["nu"], P["nb"], P["ng"])
        for key in ("A", "B", "b", "Q", "S", "R", "q", "r", "lb", "ub", "C", "D", "lg", "ug"):
            assert sv.sizes[key] == lay["sizes"][key], key
            assert np.array_equal(sv.offsets[key], lay["offsets"][key]), key
        for out, key in (("u", "u"), ("x", "x"), ("pi_out", "pi"), ("lam_out", "lam")):
            assert sv.sizes[out] == lay["sizes"][key], out
        assert np.array_equal(sv.offsets["lam_out"], lay["offsets"]["lam"])
        n1 = P["N"] + 1
        assert (sv.sizes["d"], sv.sizes["ux"], sv.sizes["pi"], sv.sizes["lam"]) == (32 * n1, 16 * n1, 16 * n1, 32 * n1)
        assert sv.sizes["res"] >= 2 * 16 * n1 + 2 * 32 * n1 + 1 and sv.sizes["N"] == P["N"]


def test_tile_plan_runs_the_existing_batched_call(refs):
    Ps = [refs("F", s)[0] for s in (1, 2, 3)]
    sv, _ = solve_batch(Ps, "C")
    outs = (sv.ux, sv.pi, sv.lam, sv.t, sv.kk, sv.ret, sv.stat)
    sv.torch.cuda.synchronize()
    a = [x.cpu().numpy().copy() for x in outs]
    assert a[4].min() > 0
    for x in outs:
        x.zero_()
    L = ocp_lib()
    tile = L.hpmpc_mi355x_ocp_tile_plan(sv.plan)
    assert tile
    rc = L.hpmpc_mi355x_ipm_batch(tile, None, sv.nprob, 0, sv.nprob, sv.BAbt.data_ptr(), sv.RSQrq.data_ptr(),
                                  sv.d.data_ptr(), sv.ux.data_ptr(), sv.pi.data_ptr(), sv.lam.data_ptr(),
                                  sv.t.data_ptr(), sv.ws.data_ptr(), sv.k_max, ARGS["mu0"], ARGS["mu_tol"],
                                  ARGS["alpha_min"], 0, 1, sv.kk.data_ptr(), sv.ret.data_ptr(), sv.stat.data_ptr(),
                                  sv._stream())
    assert rc == 0
    sv.torch.cuda.synchronize()
    for x, b in zip(outs, a):
        assert np.array_equal(x.cpu().numpy(), b)
    # with general constraints the existing call still refuses the plan
    Pg = problems("V", [1])
    sg = make_solver(Pg, "C")
    rc = L.hpmpc_mi355x_ipm_batch(L.hpmpc_mi355x_ocp_tile_plan(sg.plan), None, 1, 0, 1, sg.BAbt.data_ptr(),
                                  sg.RSQrq.data_ptr(), sg.d.data_ptr(), sg.ux.data_ptr(), sg.pi.data_ptr(),
                                  sg.lam.data_ptr(), sg.t.data_ptr(), sg.ws.data_ptr(), sg.k_max, 2.0, 1e-10, 1e-8, 0, 1,
                                  sg.kk.data_ptr(), sg.ret.data_ptr(), sg.stat.data_ptr(), sg._stream())
    assert rc == EUNSUPPORTED


# --------------------------------------------------------------------------- 11, 12: one placement for every unpack / pack
@pytest.mark.parametrize("order", ["C", "F"])
@pytest.mark.parametrize("case", ["V", "E"])
def test_finish_equals_the_one_set_unpack(case, order):
    """hpmpc_mi355x_ocp_finish_batch and hpmpc_mi355x_ocp_unpack_sets(nrhs = 1) run one kernel: on the solver's own d,
    ux, pi, lam, t they give the same u, x (equality-box fix included), pi, lam, t bit for bit, and neither writes t
    when t_out is null."""
    L = ocp_lib()
    Ps = problems(case, range(4))
    P = Ps[1]
    P["ub"][0] = P["ub"][0].copy()
    P["ub"][0][0] = P["lb"][0][0]  # input box 0 of stage 0: lb == ub
    j = int(P["hidxb"][0][0])
    assert j < P["nu"][0]
    sv = make_solver(Ps, order)
    pack_problems(sv, Ps)
    sv.solve(**ARGS)
    torch, s = sv.torch, sv.sizes
    names = (("u", "u"), ("x", "x"), ("pi", "pi_out"), ("lam", "lam_out"), ("t", "lam_out"))
    fin = {k: v.clone() for k, v in sv.finish().items()}
    assert fin["u"][1, sv.offsets["r"][0] + j].item() == P["lb"][0][0]
    new = lambda: {k: torch.full((sv.nprob, max(s[n], 1)), SENTINEL, dtype=torch.float64, device=sv.dev)
                   for k, n in names}
    ptr = lambda x: x.data_ptr()
    padded = [ptr(x) for x in (sv.d, sv.ux, sv.pi, sv.lam, sv.t)]

    def unpack(o, t=True):
        return L.hpmpc_mi355x_ocp_unpack_sets(sv.plan, sv.nprob, 0, sv.nprob, 1, *padded, ptr(o["u"]), ptr(o["x"]),
                                              ptr(o["pi"]), ptr(o["lam"]), ptr(o["t"]) if t else None, sv._stream())

    def finish(o, t=True):
        return L.hpmpc_mi355x_ocp_finish_batch(sv.plan, sv.nprob, 0, sv.nprob, ptr(sv.BAbt), ptr(sv.RSQrq), ptr(sv.DCt),
                                               *padded, ptr(sv.res), ptr(o["u"]), ptr(o["x"]), ptr(o["pi"]),
                                               ptr(o["lam"]), ptr(o["t"]) if t else None, ptr(sv.inf_norm_res),
                                               sv._stream())

    for call in (unpack, finish):
        for with_t in (True, False):
            o = new()
            assert call(o, with_t) == 0, (call.__name__, with_t)
            torch.cuda.synchronize()
            for k, n in names:
                got = o[k][:, :s[n]].cpu().numpy()
                if k == "t" and not with_t:
                    assert bool((o[k] == SENTINEL).all()), call.__name__
                else:
                    assert s[n] > 0 and np.array_equal(_bits(got), _bits(fin[k].cpu().numpy())), (call.__name__, k)
                assert bool((o[k][:, s[n]:] == SENTINEL).all())


def test_pack_vectors_tail_group():
    """Three stages: the four-stages-per-workgroup group of hk_ocp_pack_vectors has one idle wave.  On NaN-prefilled
    arrays after a full pack, pack(matrices=False) writes exactly the b row, the r / q row and d."""
    Ps = problems("R", range(5))
    sv = make_solver(Ps, "C")
    pack_problems(sv, Ps)
    full = packed_host(sv)
    for x in (sv.BAbt, sv.RSQrq, sv.d):
        x.fill_(float("nan"))
    pack_problems(sv, Ps, matrices=False)
    got = packed_host(sv)
    for p, P in enumerate(Ps):
        want = expected_packed(sv, P)
        assert np.array_equal(full["d"][p], want["d"])
        assert np.array_equal(_bits(got["d"][p]), _bits(want["d"]))
        rows = {name: np.zeros(want[name].size, dtype=bool) for name in ("BAbt", "RSQrq")}
        for k in range(P["N"] + 1):
            nux, nx1 = P["nu"][k] + P["nx"][k], (P["nx"][k + 1] if k < P["N"] else 0)
            row = lambda sd, i: (nux // 4) * 4 * sd + nux % 4 + 4 * i
            for i in range(nx1):
                rows["BAbt"][sv.offsets["BAbt"][k] + row((nx1 + 1) // 2 * 2, i)] = True
            for i in range(nux):
                rows["RSQrq"][sv.offsets["RSQrq"][k] + row((nux + 1) // 2 * 2, i)] = True
        for name, m in rows.items():
            assert m.any() and not m.all()
            assert np.array_equal(full[name][p], want[name]), (p, name)
            assert np.array_equal(_bits(got[name][p][m]), _bits(want[name][m])), (p, name)
            assert np.isnan(got[name][p][~m]).all(), (p, name)  # nothing else is written

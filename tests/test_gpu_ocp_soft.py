"""The soft OCP front end (hpmpc_mi355x_ocp_soft_*, hk_ocp_soft.hip, hpmpc_amd/ocp_soft.py) on the GPU.

Inputs and their admission: tests/ocp_soft_cases.py (D, Q and the goldens' batches, admitted by
tests/test_ocp_soft_host.py) and tests/soft_cases.py (the C shapes).  Packing and unpacking are pure data movement and
are compared bit for bit; solves are compared per problem at the project's soft gates -- helpers.check_iface for the
wrapper's outputs (kk / ret identical, TOL_SOFT, inf_norm_res at 1e-7 absolute), SC.soft_errors at TOL_SOFT for the
padded iterate; the batched residual is compared bit for bit with the one-problem d_res_mpc_soft_tv of the product.
Batches hold 3 to 5 problems.
"""
import ctypes as C
import types

import numpy as np
import pytest

import ocp_soft_cases as OC
import soft_cases as SC
from helpers import TOL_SOFT, check_iface
from hpmpc_amd.bindings import lib
from hpmpc_amd.golden import load_all
from hpmpc_amd.ocp import rup
from hpmpc_amd.ocp_soft import (OcpSoftBatchSolver, flatten_soft_problems, ocp_soft_plan_create, soft_iface_from_qp)
from hpmpc_amd.soft import SoftBatchSolver, soft_batch_layout, unpack_soft_solution

pytestmark = pytest.mark.gpu
IO = OC.IO
EUNSUPPORTED = -10
NAN = float("nan")
Z_GIVEN = {"D": False, "Q": False}  # the C shapes pass z
PACK_SHAPES = ("D", "Q") + OC.C_SHAPES
RES_SHAPES = ("D", "Q", "x0_u")


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


def _same(a, b):
    a, b = np.ascontiguousarray(a), np.ascontiguousarray(b)
    return a.shape == b.shape and a.dtype == b.dtype and a.tobytes() == b.tobytes()


def with_z(shape):
    return Z_GIVEN.get(shape, True)


def dev_data(Ps, z, order="C"):
    import torch

    flat = flatten_soft_problems(Ps, order)
    if not z:
        del flat["z"]
    return {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for k, v in flat.items()}


def make_solver(Ps, z, order="C", data=None):
    P = Ps[0]
    data = dev_data(Ps, z, order) if data is None else data
    return OcpSoftBatchSolver(P["N"], P["nx"], P["nu"], P["nb"], P["hidxb"], P["ns"], data, nprob=len(Ps), order=order,
                              k_max=OC.ARGS["k_max"])


def packed_arrays(sv):
    return dict(BAbt=sv.BAbt, RSQrq=sv.RSQrq, d=sv.d, Z=sv.Zp, z=sv.zp)


def packed_host(sv):
    sv.torch.cuda.synchronize()
    n = dict(BAbt=sv.sizes["BAbt"], RSQrq=sv.sizes["RSQrq"], d=sv.sizes["d"], Z=sv.sizes["Zp"], z=sv.sizes["Zp"])
    return {k: x.cpu().numpy()[:, :n[k]] for k, x in packed_arrays(sv).items()}


def prefill(sv, value=NAN, iterate=False):
    """Everything that needs no initialisation (and, where asked, the iterate) -> ``value``."""
    xs = list(packed_arrays(sv).values()) + [sv.ws, sv.res, sv.u, sv.x, sv.pi_out, sv.lam_out, sv.t_out, sv.inf_norm_res]
    if iterate:
        xs += [sv.ux, sv.pi, sv.lam, sv.t, sv.stat]
        sv.kk.fill_(-3)
        sv.ret.fill_(-3)
    for x in xs:
        x.fill_(value)


def solve(sv, shape, **kw):
    a = OC.args_of(shape)
    sv.solve(mu0=a["mu0"], mu_tol=a["mu_tol"], alpha_min=a["alpha_min"], k_max=a["k_max"], **kw)


def run(Ps, shape, order="C"):
    sv = make_solver(Ps, with_z(shape), order)
    prefill(sv)
    sv.pack()
    solve(sv, shape)
    return sv, sv.results()


def iterate_host(sv, Ps, shape):
    """The padded iterate per problem, as HpmpcAPI.ipm_soft returns it (dicts of ux, pi, lam, t, stat, kk, ret)."""
    sv.torch.cuda.synchronize()
    n1 = sv.N + 1
    c = lambda x: x.cpu().numpy()
    stat = c(sv.stat).reshape(-1)[:sv.nprob * 5 * sv.k_max].reshape(sv.nprob, -1)
    return unpack_soft_solution(OC.soft_qp(Ps[0], with_z(shape)), c(sv.ux).reshape(-1, n1, 16),
                                c(sv.pi).reshape(-1, n1, 16), c(sv.lam)[:, :max(sv.sizes["lam"], 1)],
                                c(sv.t)[:, :max(sv.sizes["lam"], 1)], c(sv.kk), c(sv.ret), stat)


def dense_from_iterate(P, r):
    """u, x, pi and the compact lam / t the wrapper returns for the padded iterate ``r``."""
    N, nu, nx, nb, ns = P["N"], P["nu"], P["nx"], P["nb"], P["ns"]
    out = dict(u=[r["ux"][k][:nu[k]] for k in range(N)], x=[r["ux"][k][nu[k]:nu[k] + nx[k]] for k in range(N + 1)],
               pi=[r["pi"][k][:nx[k + 1]] for k in range(N)], lam=[], t=[])
    for k in range(N + 1):
        pnb, pns = rup(nb[k], 4), rup(ns[k], 4)
        for key in ("lam", "t"):
            v = r[key][k]
            out[key].append(np.concatenate([v[:nb[k]], v[pnb:pnb + nb[k]]] +
                                           [v[2 * pnb + s * pns:2 * pnb + s * pns + ns[k]] for s in range(4)]))
    return out


def assert_outputs_are_the_iterate(P, got, r, tag):
    want = dense_from_iterate(P, r)
    for key in ("u", "x", "pi", "lam", "t"):
        assert len(got[key]) == len(want[key]), (tag, key)
        for k, (g, w) in enumerate(zip(got[key], want[key])):
            assert np.array_equal(_bits(g), _bits(w)), (tag, key, k)


def wrapper_norms(P, res):
    """max |r_q|, |r_b|, |r_d| over the elements fortran_order_d_ip_ocp_soft_tv visits, from 0."""
    N, nu, nx, nb, ns = P["N"], P["nu"], P["nx"], P["nb"], P["ns"]
    mx = lambda v: float(np.max(np.abs(v), initial=0.0))
    tq = max(mx(res["rq"][k][:nu[k] + nx[k]]) for k in range(N + 1))
    tb = max(mx(res["rb"][k][:nx[k + 1]]) for k in range(N))
    td = 0.0
    for k in range(N + 1):
        pnb, pns = rup(nb[k], 4), rup(ns[k], 4)
        idx = np.r_[0:nb[k], pnb:pnb + nb[k], 2 * pnb:2 * pnb + ns[k], 2 * pnb + pns:2 * pnb + pns + ns[k]].astype(int)
        td = max(td, mx(np.asarray(res["rd"][k])[idx]))
    return np.array([tq, tb, td])


def res_q(P):
    return [np.r_[P["r"][k] if k < P["N"] else [], P["q"][k], np.zeros(8)] for k in range(P["N"] + 1)]


@pytest.fixture(scope="module")
def solved():
    """One pack -> solve -> finish per shape, shared by the tests that only read it."""
    cache = {}

    def get(shape):
        if shape not in cache:
            Ps = OC.problems(shape)
            sv, got = run(Ps, shape)
            cache[shape] = (Ps, sv, got, iterate_host(sv, Ps, shape))
        return cache[shape]

    return get


@pytest.fixture(scope="module")
def refs(oracle):
    """The oracle's answers, computed once per shape and shared (never modified)."""
    cache = {}

    def get(shape):
        if shape not in cache:
            Ps = OC.problems(shape)
            a = OC.args_of(shape)
            if with_z(shape):
                cache[shape] = [oracle.ipm_soft(OC.soft_qp(P, True), **a) for P in Ps]
            else:
                cache[shape] = [IO.ip_ocp_soft(oracle, P, k_max=a["k_max"], mu0=a["mu0"], mu_tol=a["mu_tol"]) for P in Ps]
        return cache[shape]

    return get


# ------------------------------------------------------------------------------------------------------------ 1: pack
@pytest.mark.parametrize("shape", PACK_SHAPES)
def test_pack_is_bitwise(shape):
    Ps = OC.problems(shape)
    assert 3 <= len(Ps) <= 5
    sv = make_solver(Ps, with_z(shape))
    lay = soft_batch_layout(OC.soft_qp(Ps[0], False))["sizes"]
    assert (sv.sizes["d"], sv.sizes["Zp"], sv.sizes["lam"], sv.sizes["ux"], sv.sizes["ws"]) == \
        (lay["d"], lay["Z"], lay["C"], lay["ux"], lay["ws"])
    prefill(sv)
    sv.pack()
    got, want = packed_host(sv), OC.expected_packed(Ps, with_z(shape))
    for name in want:
        assert got[name].shape == want[name].shape, name
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name
    assert bool(want["z"].any()) == with_z(shape)  # a null z packs zeros, a given one is packed like Z
    if shape == "full16":
        assert max(rup(b, 4) + rup(s, 4) for b, s in zip(Ps[0]["nb"], Ps[0]["ns"])) > 16


# ------------------------------------------------------------------------------------------- 2: against the reference
@pytest.mark.parametrize("name", list(OC.GOLDENS))
def test_golden_inside_a_batch(name):
    case = {c.name: c for c in load_all()}[name]
    qp = case.qp
    Ps = OC.problems(name)
    at = OC.GOLDEN_AT
    Pg = IO.from_flat(qp.N, qp.nx, qp.nu, qp.nb, qp.ng, case.inp)
    for key in ("A", "Q", "lb", "Z"):  # the golden's inputs are this shape's draw at the golden's seed
        assert all(np.array_equal(a, b) for a, b in zip(Pg[key], Ps[at][key])), key
    assert (float(case.args["mu0"]), float(case.args["mu_tol"]), int(case.args["k_max"])) == \
        (OC.args_of(name)["mu0"], OC.ARGS["mu_tol"], OC.ARGS["k_max"])
    Ps[at] = Pg
    sv = make_solver(Ps, False)
    prefill(sv)
    sv.pack()
    solve(sv, name)
    got = sv.results()
    assert sv.res_ok and [g["kk"] for g in got] == OC.kks(name)
    g = dict(got[at], ret=got[at]["status"])
    print(name, "kk", g["kk"], "inf_norm_res", g["inf_norm_res"], "golden", case.out["inf_norm_res"])
    check_iface(case, g)


# ---------------------------------------------------------------------------------------------- 3: against the oracle
@pytest.mark.parametrize("shape", ["D", "Q"])
def test_wrapper_outputs_vs_oracle(solved, refs, shape):
    Ps, sv, got, it = solved(shape)
    ref = refs(shape)
    assert sv.res_ok and [r["kk"] for r in ref] == OC.kks(shape) and all(r["status"] == 0 for r in ref)
    for p, (P, g, r) in enumerate(zip(Ps, got, ref)):
        case = types.SimpleNamespace(kind="iface_soft", name=f"{shape}[{p}]", out=dict(r, ret=r["status"]))
        print(case.name, "kk", g["kk"], "inf_norm_res", g["inf_norm_res"], "oracle", r["inf_norm_res"])
        check_iface(case, dict(g, ret=g["status"]))
        assert_outputs_are_the_iterate(P, g, it[p], case.name)


def test_q_norms_tell_the_two_readings_apart(oracle, refs):
    """On Q the reference reads the variable of a soft constraint at idxb[nu + i]; a restatement that read it at
    idxb[nb + i] would report another max |r_d|, by more than the 1e-7 gate: the check of test 3 bites."""
    ref = refs("Q")
    a = OC.args_of("Q")
    for P, r in zip(OC.problems("Q"), ref):
        o = oracle.ipm_soft(OC.soft_qp(P, False), **a)
        as_ref, other = OC.soft_rd_max(P, o["ux"], o["t"], "nu"), OC.soft_rd_max(P, o["ux"], o["t"], "nb")
        assert abs(as_ref - r["inf_norm_res"][2]) <= 1e-12 * max(1.0, as_ref)  # the restatement is the oracle's
        assert abs(as_ref - other) > 1e-7, (as_ref, other)


@pytest.mark.parametrize("shape", OC.C_SHAPES)
def test_iterate_vs_oracle_with_z(oracle, solved, refs, shape):
    Ps, sv, got, it = solved(shape)
    ref = refs(shape)
    assert [r["kk"] for r in ref] == OC.kks(shape)
    for p, (P, g, r) in enumerate(zip(Ps, it, ref)):
        sq = OC.soft_qp(P, True)
        share = SC.gate_share(SC.soft_errors(sq, g, r))
        print(f"{shape}[{p}]: kk {g['kk']} ret {g['ret']}, share of gate " + " ".join(f"{k} {v:.2e}" for k, v in share.items()))
        assert max(share.values()) <= 1.0, (shape, p, share)
        assert_outputs_are_the_iterate(P, got[p], g, (shape, p))
        assert (got[p]["kk"], got[p]["status"]) == (r["kk"], r["ret"])
    assert sv.res_ok == (shape == "x0_u")
    if shape == "x0_u":
        # the oracle's residual at the product's iterate: the same inputs, so the norms differ by rounding alone --
        # sums of at most 40 terms below 1e3 in magnitude, 40 * 1e3 * 2^-53 < 1e-11; mu likewise
        for p, (P, g) in enumerate(zip(Ps, it)):
            res = oracle.residuals_soft(OC.soft_qp(P, True), res_q(P), g["ux"], g["pi"], g["lam"], g["t"])
            want = np.r_[wrapper_norms(P, res), res["mu"]]
            print(f"x0_u[{p}] inf_norm_res", got[p]["inf_norm_res"], "oracle", want)
            np.testing.assert_allclose(got[p]["inf_norm_res"], want, rtol=0, atol=1e-9)
    else:
        assert "inf_norm_res" not in got[0]


# ------------------------------------------------------------------------------------- 4: same kernel, same answer
@pytest.mark.parametrize("shape", OC.C_SHAPES)
def test_same_answer_as_soft_batch_solver(solved, shape):
    Ps, sv, _, _ = solved(shape)
    ref = SoftBatchSolver([OC.soft_qp(P, True) for P in Ps], k_max=OC.ARGS["k_max"])
    ref.solve(**OC.ARGS)
    ref.torch.cuda.synchronize()
    c = lambda x: x.cpu().numpy()
    n = sv.sizes["lam"]
    assert int(c(ref.kk).max()) > 0
    for name, a, b in (("ux", sv.ux, ref.ux), ("pi", sv.pi, ref.pi), ("lam", sv.lam[:, :n], ref.lam[:, :n]),
                       ("t", sv.t[:, :n], ref.t[:, :n]), ("kk", sv.kk, ref.kk), ("ret", sv.ret, ref.ret),
                       ("stat", sv.stat, ref.stat)):
        assert _same(c(a).reshape(len(Ps), -1), c(b).reshape(len(Ps), -1)), (shape, name)


# ------------------------------------------------------------------------------------------------ 5: residual parity
@pytest.mark.parametrize("shape", RES_SHAPES)
def test_residual_is_the_one_problem_entry_point(product, solved, shape):
    Ps, sv, got, it = solved(shape)
    assert sv.res_ok
    N, n1 = sv.N, sv.N + 1
    res = sv.res.cpu().numpy()
    sRes = sv.sizes["res"] - 8
    img = res.reshape(-1)[:sv.nprob * sRes].reshape(sv.nprob, sRes)
    mu = res.reshape(-1)[sv.nprob * sRes:sv.nprob * sRes + sv.nprob]
    oD, oZ, sD = sv.offsets["d"], sv.offsets["Zp"], sv.sizes["d"]
    inf = sv.inf_norm_res.cpu().numpy()
    for p, (P, g) in enumerate(zip(Ps, it)):
        one = product.residuals_soft(OC.soft_qp(P, with_z(shape)), res_q(P), g["ux"], g["pi"], g["lam"], g["t"])
        terms = 0
        for k in range(n1):
            nux, nb, ns = P["nu"][k] + P["nx"][k], P["nb"][k], P["ns"][k]
            pnb, pns = rup(nb, 4), rup(ns, 4)
            assert np.array_equal(_bits(img[p, 16 * k:16 * k + nux]), _bits(one["rq"][k][:nux])), (p, "rq", k)
            if k < N:
                nx1 = P["nx"][k + 1]
                assert np.array_equal(_bits(img[p, 16 * (n1 + k):16 * (n1 + k) + nx1]), _bits(one["rb"][k][:nx1])), (p, "rb", k)
            live = np.r_[0:nb, pnb:pnb + nb, 2 * pnb:2 * pnb + ns, 2 * pnb + pns:2 * pnb + pns + ns].astype(int)
            rd = img[p, 32 * n1 + oD[k]:32 * n1 + oD[k] + 2 * pnb + 2 * pns]
            assert np.array_equal(_bits(rd[live]), _bits(np.asarray(one["rd"][k])[live])), (p, "rd", k)
            lz = np.r_[0:ns, pns:pns + ns].astype(int)
            rz = img[p, 32 * n1 + sD + oZ[k]:32 * n1 + sD + oZ[k] + 2 * pns]
            assert np.array_equal(_bits(rz[lz]), _bits(np.asarray(one["rz"][k])[lz])), (p, "rz", k)
            terms += 2 * nb + 4 * ns
        assert np.array_equal(_bits(inf[p, :3]), _bits(wrapper_norms(P, one))), (p, inf[p], wrapper_norms(P, one))
        # mu sums `terms` positive products lam t: a reordered sum moves by at most terms * eps relative
        assert inf[p, 3] == mu[p] and abs(mu[p] - one["mu"]) <= terms * np.finfo(float).eps * abs(one["mu"]), (p, mu[p], one["mu"])
        assert np.array_equal(_bits(got[p]["inf_norm_res"]), _bits(inf[p]))


# ----------------------------------------------------------------------------------------------- 6: receding horizon
def _next_step(Ps, seed=5):
    """The same problems one step on: b_0, q, r and the bounds change, the matrices do not."""
    rng = np.random.default_rng(seed)
    out = []
    for P in Ps:
        Q = {k: ([np.array(a, copy=True) for a in v] if isinstance(v, list) else v) for k, v in P.items()}
        Q["b"][0] = P["b"][0] + 0.05 * rng.standard_normal(P["b"][0].shape)
        for key in ("q", "r"):
            Q[key] = [v + 0.05 * rng.standard_normal(v.shape) for v in P[key]]
        Q["lb"] = [v - 0.05 * rng.random(v.shape) for v in P["lb"]]
        Q["ub"] = [v + 0.05 * rng.random(v.shape) for v in P["ub"]]
        out.append(Q)
    return out


@pytest.mark.parametrize("shape", ["D", "odd"])
def test_vectors_only_repack(shape):
    first = OC.problems(shape)
    second = _next_step(first)
    z = with_z(shape)
    sv = make_solver(first, z)
    prefill(sv)
    sv.pack()
    before = packed_host(sv)
    new = dev_data(second, z)
    sv.pack(matrices=False, data={k: new[k] for k in ("b", "q", "r", "lb", "ub")})
    got, want = packed_host(sv), OC.expected_packed(second, z)
    for name in want:
        assert np.array_equal(_bits(got[name]), _bits(want[name])), name
    assert not np.array_equal(before["BAbt"], got["BAbt"]) and not np.array_equal(before["d"], got["d"])


def test_warm_start_is_set_ux(solved):
    import torch

    shape = "x0_u"
    Ps, cold, _, it = solved(shape)
    dense = [dense_from_iterate(P, r) for P, r in zip(Ps, it)]
    stack = lambda key: torch.from_numpy(np.stack([np.concatenate([0.9 * v for v in d[key]]) for d in dense])).to("cuda")
    sv = make_solver(Ps, True)
    prefill(sv)
    sv.ux.fill_(NAN)  # every element of ux is written, padding as zeros
    sv.pack(warm=dict(u=stack("u"), x=stack("x")))
    ref = SoftBatchSolver([OC.soft_qp(P, True) for P in Ps], k_max=OC.ARGS["k_max"])
    ref.set_ux([[0.9 * np.asarray(v) for v in r["ux"]] for r in it])
    c = lambda x: x.cpu().numpy().reshape(len(Ps), -1)
    assert _same(c(sv.ux), c(ref.ux))
    solve(sv, shape, warm_start=1)
    ref.solve(warm_start=1, **OC.ARGS)
    sv.torch.cuda.synchronize()
    n = sv.sizes["lam"]
    assert int(c(ref.kk).max()) > 0
    for name, a, b in (("ux", sv.ux, ref.ux), ("pi", sv.pi, ref.pi), ("lam", sv.lam[:, :n], ref.lam[:, :n]),
                       ("t", sv.t[:, :n], ref.t[:, :n]), ("kk", sv.kk, ref.kk), ("ret", sv.ret, ref.ret),
                       ("stat", sv.stat, ref.stat)):
        assert _same(c(a), c(b)), name


# --------------------------------------------------------------------------------------------- 7: ranges and sharing
def test_sub_range_leaves_the_rest(solved):
    Ps, full, got_full, _ = solved("D")
    assert len(Ps) == 4
    sv = make_solver(Ps, False)
    prefill(sv, iterate=True)
    sv.pack(p0=1, count=2)
    a = OC.args_of("D")
    sv.solve(mu0=a["mu0"], mu_tol=a["mu_tol"], alpha_min=a["alpha_min"], p0=1, count=2)
    out = sv.finish(p0=1, count=2)
    sv.torch.cuda.synchronize()
    arrays = dict(packed_arrays(sv), ux=sv.ux, pi=sv.pi, lam=sv.lam, t=sv.t, stat=sv.stat, u=sv.u, x=sv.x,
                  pi_out=sv.pi_out, lam_out=sv.lam_out, t_out=sv.t_out, inf=sv.inf_norm_res)
    twin = dict(packed_arrays(full), ux=full.ux, pi=full.pi, lam=full.lam, t=full.t, stat=full.stat, u=full.u, x=full.x,
                pi_out=full.pi_out, lam_out=full.lam_out, t_out=full.t_out, inf=full.inf_norm_res)
    for name, x in arrays.items():
        h, f = x.cpu().numpy(), twin[name].cpu().numpy()
        for p in (0, 3):
            assert np.isnan(h[p]).all(), (name, p)
        if name in ("ux", "pi", "lam", "t", "stat"):
            continue  # their padding is never written: the iterate is compared through the outputs
        for p in (1, 2):
            assert np.array_equal(_bits(h[p]), _bits(f[p])), (name, p)
    assert sv.kk.tolist()[0] == sv.kk.tolist()[3] == -3 and sv.ret.tolist()[0] == sv.ret.tolist()[3] == -3
    assert sv.kk.tolist()[1:3] == full.kk.tolist()[1:3]
    assert "inf_norm_res" in out


def test_shared_arrays_are_replicated_copies():
    Ps = OC.problems("Q")
    for P in Ps[1:]:  # one set of matrices and penalties for the whole batch
        for key in ("A", "B", "Q", "S", "R", "Z"):
            P[key] = Ps[0][key]
    data = dev_data(Ps, False)
    sv = make_solver(Ps, False, data=dict(data))
    prefill(sv)
    sv.pack()
    full = packed_host(sv)
    for key in ("A", "B", "Q", "S", "R", "Z"):
        data[key] = data[key][0].clone()  # no batch dimension: stride 0
        assert data[key].dim() == 1
    prefill(sv)
    sv.pack(data=data)
    shared, want = packed_host(sv), OC.expected_packed(Ps, False)
    for name in want:
        assert np.array_equal(_bits(shared[name]), _bits(full[name])), name
        assert np.array_equal(_bits(shared[name]), _bits(want[name])), name


@pytest.mark.parametrize("shape", ["Q", "odd"])
def test_row_major_equals_column_major(shape):
    Ps = OC.problems(shape)
    out = []
    for order in ("F", "C"):
        sv = make_solver(Ps, with_z(shape), order)
        prefill(sv)
        sv.pack()
        out.append(packed_host(sv))
    flat = {o: flatten_soft_problems(Ps, o) for o in ("F", "C")}
    assert not np.array_equal(flat["F"]["A"], flat["C"]["A"])  # the blocks really are transposed
    for name in out[0]:
        assert np.array_equal(_bits(out[0][name]), _bits(out[1][name])), name


# ------------------------------------------------------------------------------------------------------- 8: refusals
def test_plan_refusals():
    P = OC.make("D", 0)
    N = P["N"]
    ok, err, _ = ocp_soft_plan_create(N, P["nx"], P["nu"], P["nb"], P["hidxb"], P["ns"])
    assert ok and err == 0
    lib().hpmpc_mi355x_ocp_soft_plan_destroy(ok)
    ng = [0] * (N + 1)
    ng[2] = 1
    plan, err, _ = ocp_soft_plan_create(N, P["nx"], P["nu"], P["nb"], P["hidxb"], P["ns"], ng=ng)
    assert plan is None and err == EUNSUPPORTED
    R = soft_iface_from_qp(SC.refusal_shape())  # the stray soft-gradient write into a live Zl
    plan, err, _ = ocp_soft_plan_create(R["N"], R["nx"], R["nu"], R["nb"], R["hidxb"], R["ns"])
    assert plan is None and err == EUNSUPPORTED
    ns = list(P["ns"])
    ns[1] = P["nu"][1] + P["nx"][1] - P["nb"][1] + 1  # nb + ns > nu + nx
    idx = [np.arange(16, dtype=np.int32) for _ in range(N + 1)]
    plan, err, _ = ocp_soft_plan_create(N, P["nx"], P["nu"], P["nb"], idx, ns)
    assert plan is None and err == EUNSUPPORTED


def test_call_refusals_write_nothing():
    Ps = OC.problems("Q")
    sv = make_solver(Ps, False)
    L = lib()
    prefill(sv, value=-7.25, iterate=True)
    state = list(packed_arrays(sv).values()) + [sv.ux, sv.pi, sv.lam, sv.t, sv.stat, sv.res, sv.u, sv.x, sv.pi_out,
                                                sv.lam_out, sv.t_out, sv.inf_norm_res]
    ds = sv.data_struct()
    p = lambda x, given=True: x.data_ptr() if given else None

    def pack(BAbt=True, p0=0, count=sv.nprob):
        return L.hpmpc_mi355x_ocp_soft_pack_batch(sv.plan, C.byref(ds), 1, sv.nprob, p0, count, p(sv.BAbt, BAbt),
                                                  p(sv.RSQrq), p(sv.d), p(sv.Zp), p(sv.zp), None, None, None, sv._stream())

    def ipm(mu0, lam=True):
        return L.hpmpc_mi355x_ocp_soft_ipm_batch(sv.plan, sv.nprob, 0, sv.nprob, *sv._packed(), p(sv.ux), p(sv.pi),
                                                 p(sv.lam, lam), p(sv.t), p(sv.ws), sv.k_max, mu0, 1e-6, 1e-8, 0, 1,
                                                 p(sv.kk), p(sv.ret), p(sv.stat), sv._stream())

    def finish(u=True, p0=0, count=sv.nprob):
        return L.hpmpc_mi355x_ocp_soft_finish_batch(sv.plan, sv.nprob, p0, count, *sv._packed(), p(sv.ux), p(sv.pi),
                                                    p(sv.lam), p(sv.t), p(sv.res), p(sv.u, u), p(sv.x), p(sv.pi_out),
                                                    p(sv.lam_out), p(sv.t_out), p(sv.inf_norm_res), sv._stream())

    for call in (lambda: pack(BAbt=False), lambda: pack(p0=1, count=sv.nprob), lambda: pack(p0=-1, count=1),
                 lambda: ipm(0.0), lambda: ipm(-1.0), lambda: ipm(100.0, lam=False), lambda: finish(u=False),
                 lambda: finish(p0=2, count=sv.nprob)):
        assert call() == EUNSUPPORTED
        assert L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    for call in (lambda: pack(count=0), lambda: finish(count=0), lambda: pack(BAbt=False, count=0)):
        assert call() == 0 and L.hpmpc_mi355x_last_error() == 0  # an empty range asks for no array
    with pytest.raises(RuntimeError):
        sv.solve(mu0=0.0)
    sv.torch.cuda.synchronize()
    for x in state:
        assert bool((x == -7.25).all())
    assert sv.kk.tolist() == [-3] * sv.nprob and sv.ret.tolist() == [-3] * sv.nprob


def test_norms_are_refused_without_res_ok(solved):
    Ps, sv, got, it = solved("softonly")
    assert not sv.res_ok and "inf_norm_res" not in got[0]
    L = lib()
    sv.torch.cuda.synchronize()
    outs = (sv.u, sv.x, sv.pi_out, sv.lam_out, sv.t_out, sv.inf_norm_res, sv.res)
    for x in outs:
        x.fill_(-7.25)
    rc = L.hpmpc_mi355x_ocp_soft_finish_batch(
        sv.plan, sv.nprob, 0, sv.nprob, *sv._packed(), sv.ux.data_ptr(), sv.pi.data_ptr(), sv.lam.data_ptr(),
        sv.t.data_ptr(), sv.res.data_ptr(), sv.u.data_ptr(), sv.x.data_ptr(), sv.pi_out.data_ptr(),
        sv.lam_out.data_ptr(), sv.t_out.data_ptr(), sv.inf_norm_res.data_ptr(), sv._stream())
    assert rc == EUNSUPPORTED and L.hpmpc_mi355x_last_error() == EUNSUPPORTED
    with pytest.raises(ValueError):
        sv.finish(norms=True)
    sv.torch.cuda.synchronize()
    for x in outs:
        assert bool((x == -7.25).all())
    again = sv.results(sv.finish())  # null norms: the finish works, and gives test 4's iterate
    for p, (P, g) in enumerate(zip(Ps, again)):
        assert "inf_norm_res" not in g
        assert_outputs_are_the_iterate(P, g, it[p], p)
    assert bool((sv.inf_norm_res == -7.25).all()) and bool((sv.res == -7.25).all())

"""The soft OCP front end (hpmpc_mi355x_ocp_soft_*, hpmpc_amd/ocp_soft.py) on the CPU: the host helper that turns a
SoftQP into the interface form, the admission rule on every new input of tests/test_gpu_ocp_soft.py, and the agreement
of the header, the export map and the binding table on the new symbols."""
import fnmatch
import os
import re

import numpy as np
import pytest

import ocp_soft_cases as OC
import soft_cases as SC
from hpmpc_amd import bindings
from hpmpc_amd.ocp_soft import (KEYS, flatten_soft_problems, soft_dense_layout, soft_iface_from_qp,
                                unflatten_soft_outputs)

IO = OC.IO
ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ["hpmpc_mi355x_ocp_soft_plan_create", "hpmpc_mi355x_ocp_soft_plan_destroy", "hpmpc_mi355x_ocp_soft_ipm_plan",
       "hpmpc_mi355x_ocp_soft_sizes", "hpmpc_mi355x_ocp_soft_offsets", "hpmpc_mi355x_ocp_soft_pack_batch",
       "hpmpc_mi355x_ocp_soft_ipm_batch", "hpmpc_mi355x_ocp_soft_finish_batch"]


def _bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.int64)


@pytest.fixture(scope="module")
def oracle_fma(oracle):  # after `oracle`: that fixture builds both libraries where they are missing
    from hpmpc_amd.cabi import HpmpcAPI, load

    return HpmpcAPI(load(os.path.join(ROOT, "oracle", "liboracle_fma.so")), "orc_")


@pytest.mark.parametrize("name", list(SC.CASES))
def test_iface_round_trip_is_bitwise(name):
    """to_soft_qp(soft_iface_from_qp(sq)) is sq: BAbt, RSQrq, d, Z and idxb bit for bit (and z, once filled as the
    front end packs a given z), on every admitted draw."""
    for seed in SC.seeds(name):
        sq = SC.make(name, seed)
        P = soft_iface_from_qp(sq)
        assert P["ng"] == [0] * (sq.N + 1) and P["nu"][sq.N] == 0
        back = IO.to_soft_qp(P)
        for f in ("nx", "nu", "nb", "ns"):
            assert np.array_equal(getattr(back, f), getattr(sq, f)), f
        for k in range(sq.N + 1):
            assert back.idxb[k].dtype == sq.idxb[k].dtype and np.array_equal(back.idxb[k], sq.idxb[k]), k
            for f in ("RSQrq", "d", "Z") + (("BAbt",) if k < sq.N else ()):
                a, b = getattr(back, f)[k], getattr(sq, f)[k]
                assert a.shape == b.shape and np.array_equal(_bits(a), _bits(b)), (seed, f, k)
            assert not back.z[k].any()  # the reference wrapper's z
            z = OC.soft_qp(P, True).z[k]
            assert z.shape == sq.z[k].shape and np.array_equal(_bits(z), _bits(sq.z[k])), (seed, "z", k)


def test_flatten_layout():
    """flatten_soft_problems puts every stage block at soft_dense_layout's offsets, lb / ub with nb + ns entries and
    Z / z with 2 ns; the outputs come back by the same table."""
    Ps = OC.problems("Q")
    N, nx, nu, nb, ns = (Ps[0][k] for k in ("N", "nx", "nu", "nb", "ns"))
    lay = soft_dense_layout(N, nx, nu, nb, ns)
    assert lay["sizes"]["lb"] == sum(nb) + sum(ns) and lay["sizes"]["Z"] == 2 * sum(ns)
    assert lay["sizes"]["lam"] == 2 * sum(nb) + 4 * sum(ns) and lay["sizes"]["u"] == sum(nu)
    for order in ("C", "F"):
        flat = flatten_soft_problems(Ps, order)
        assert set(flat) == set(KEYS)
        for p, P in enumerate(Ps):
            for key in KEYS:
                for k, M in enumerate(P[key]):
                    o = lay["offsets"][key][k]
                    assert np.array_equal(flat[key][p, o:o + M.size], np.asarray(M).flatten(order)), (key, k)
    rng = np.random.default_rng(0)
    outs = {key: rng.standard_normal((2, lay["sizes"][key])) for key in ("u", "x", "pi", "lam", "t")}
    per = unflatten_soft_outputs(outs, N, nx, nu, nb, ns)
    assert [len(per[1][key]) for key in ("u", "x", "pi", "lam", "t")] == [N, N + 1, N, N + 1, N + 1]
    for key in outs:
        assert np.array_equal(np.concatenate(per[1][key]), outs[key][1])


def test_q_shape_separates_the_two_readings():
    """Q: res_ok holds (nu <= nb wherever ns > 0, k < N) and on stage 1 idxb[nu + i] != idxb[nb + i] for every i."""
    P = OC.make("Q", OC.seeds("Q")[0])
    N = P["N"]
    assert all(P["nu"][k] <= P["nb"][k] for k in range(N) if P["ns"][k] > 0)
    ib, nu, nb, ns = P["hidxb"][1], P["nu"][1], P["nb"][1], P["ns"][1]
    assert nb > nu and ns > 0 and all(ib[nu + i] != ib[nb + i] for i in range(ns))
    assert not SC.soft_stray_targets(IO.to_soft_qp(P))[1]


@pytest.mark.parametrize("shape", list(OC.DRAWS))
def test_admission_rule_holds(oracle, oracle_fma, shape):
    """Every pinned (shape, seed) of D, Q and the goldens' batches: the two oracle builds agree on kk / ret (the pins),
    differ by at most ADMIT of every TOL_SOFT gate, and the run converges; where the reference's c99 build is there
    (oracle/_ref), it agrees on kk / ret too."""
    from hpmpc_amd.cabi import HpmpcAPI, load

    draws = OC.DRAWS[shape]
    assert 3 <= len(draws) <= 5
    refpath = os.path.join(ROOT, "oracle", "_ref", "libhpmpc_ref.so")
    ref = HpmpcAPI(load(refpath)) if os.path.exists(refpath) else None
    a = OC.args_of(shape)
    for seed, kk, ret, _ in draws:
        sq = OC.soft_qp(OC.make(shape, seed), False)
        o, f = oracle.ipm_soft(sq.copy(), **a), oracle_fma.ipm_soft(sq.copy(), **a)
        assert (o["kk"], o["ret"]) == (f["kk"], f["ret"]) == (kk, ret), (shape, seed, o["kk"], o["ret"], f["kk"], f["ret"])
        share = SC.gate_share(SC.soft_errors(sq, f, o))
        print(f"{shape} seed {seed}: kk {kk} ret {ret}, spread " + " ".join(f"{k} {v:.1e}" for k, v in share.items()))
        assert max(share.values()) <= SC.ADMIT, (shape, seed, share)
        assert ret == 0, (shape, seed)
        if ref is not None:
            r = ref.ipm_soft(sq.copy(), work_extra=1 << 16, **a)
            assert (r["kk"], r["ret"]) == (kk, ret), (shape, seed, r["kk"], r["ret"])
    if shape in OC.GOLDENS:
        assert draws[OC.GOLDEN_AT][0] == OC.GOLDENS[shape][1]


def test_c_shapes_are_admitted_draws():
    """The C shapes are draws of tests/soft_cases.py, admitted there; each batch holds 3 to 5 problems."""
    for name in OC.C_SHAPES:
        assert name in SC.CASES and 3 <= len(SC.seeds(name)) <= 5
        assert all(d[2] == 0 for d in SC.CASES[name]["draws"])


def test_header_export_map_and_bindings_agree_on_the_new_functions():
    header = open(os.path.join(ROOT, "include", "hpmpc_mi355x.h")).read()
    text = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "typedef struct hpmpc_mi355x_ocp_soft_plan hpmpc_mi355x_ocp_soft_plan;" in text
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, text), name
        assert name in bindings.SIGNATURES, name
    assert sorted(n for n in bindings.SIGNATURES if n.startswith("hpmpc_mi355x_ocp_soft_")) == sorted(NEW)
    nargs = lambda name: len(re.search(r"\b%s\s*\(([^;]*)\)\s*;" % name, text).group(1).split(","))
    for name in NEW:
        assert nargs(name) == len(bindings.SIGNATURES[name][1]), name
    assert nargs("hpmpc_mi355x_ocp_soft_pack_batch") == 15 and nargs("hpmpc_mi355x_ocp_soft_finish_batch") == 21
    emap = open(os.path.join(ROOT, "hpmpc_amd", "csrc", "exports.map")).read()
    emap = re.sub(r"/\*.*?\*/", "", emap, flags=re.S)
    glob = re.search(r"global:(.*?)local:", emap, flags=re.S).group(1)
    patterns = [p.strip() for p in glob.split(";") if p.strip()]
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
    # the z extension and the res_ok rule are stated beside the prototypes
    assert "THE LINEAR PENALTY z" in header and "res_ok" in header
    sizes = int(re.search(r"#define HPMPC_MI355X_OCP_SOFT_NSIZES (\d+)", header).group(1))
    offs = int(re.search(r"#define HPMPC_MI355X_OCP_SOFT_NOFFSETS (\d+)", header).group(1))
    from hpmpc_amd import ocp_soft

    assert (sizes, offs) == (ocp_soft.NSIZES, ocp_soft.NOFFSETS)

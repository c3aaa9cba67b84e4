"""Host side of the batched OCP front end (hpmpc_amd/ocp_batch.py, include/hpmpc_mi355x.h): the dense layout, the
flatten / unflatten helpers and the public symbols.  No GPU and no library load."""
import fnmatch
import os
import re
import sys

import numpy as np
import pytest

from hpmpc_amd.ocp_batch import KEYS, flatten_problems, ocp_dense_layout, unflatten_problems
from ocp_batch_cases import CASES

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import iface_oracle as IO  # noqa: E402

NEW = ("hpmpc_mi355x_ocp_plan_create", "hpmpc_mi355x_ocp_plan_destroy", "hpmpc_mi355x_ocp_tile_plan",
       "hpmpc_mi355x_ocp_sizes", "hpmpc_mi355x_ocp_offsets", "hpmpc_mi355x_ocp_pack_batch",
       "hpmpc_mi355x_ocp_ipm_batch", "hpmpc_mi355x_ocp_finish_batch")
# N, nx, nu, boxed inputs, boxed states, ng
V = (5, [0, 3, 3, 5, 5, 4], [2, 2, 1, 3, 3], 2, 2, [0, 0, 2, 0, 3, 2])
F = (4, [0, 8, 8, 8, 8], [3, 3, 3, 3], 3, 4, None)
H, E, B = (CASES[c] for c in "HEB")  # the (4, 12) class, the 16-wide tile edge, all boxes


@pytest.mark.parametrize("case", [V, F, H, E, B], ids=["V", "F", "H", "E", "B"])
@pytest.mark.parametrize("order", ["C", "F"])
def test_flatten_round_trip_is_exact(case, order):
    Ps = [IO.random_iface_problem(*case, seed=s) for s in (1, 2, 3)]
    P0 = Ps[0]
    flat = flatten_problems(Ps, order)
    lay = ocp_dense_layout(P0["N"], P0["nx"], P0["nu"], P0["nb"], P0["ng"])
    for key in KEYS:
        assert flat[key].shape == (3, lay["sizes"][key]), key
    assert not np.array_equal(flat["A"][0], flat["A"][1])
    back = unflatten_problems(flat, P0["N"], P0["nx"], P0["nu"], P0["nb"], P0["ng"], order)
    assert len(back) == 3
    for P, B in zip(Ps, back):
        for key in KEYS:
            assert len(B[key]) == len(P[key]), key
            for k, (a, b) in enumerate(zip(P[key], B[key])):
                assert np.asarray(a).shape == b.shape and np.array_equal(a, b), (key, k)
    # the two orders differ exactly by the transposition of every matrix block
    other = flatten_problems(Ps, "F" if order == "C" else "C")
    assert np.array_equal(other["b"], flat["b"]) and not np.array_equal(other["A"], flat["A"])
    k, o = 2, lay["offsets"]["A"][2]
    shp = (P0["nx"][k + 1], P0["nx"][k])
    assert np.array_equal(flat["A"][1, o:o + shp[0] * shp[1]].reshape(shp, order=order), Ps[1]["A"][k])


def test_flatten_outputs_round_trip():
    N, nx, nu, bu, bx, ng = V
    P = IO.random_iface_problem(*V, seed=1)
    rng = np.random.default_rng(0)
    lay = ocp_dense_layout(N, nx, nu, P["nb"], ng)
    flat = {key: rng.standard_normal((2, lay["sizes"][key])) for key in ("u", "x", "pi", "lam", "t")}
    per = unflatten_problems(flat, N, nx, nu, P["nb"], ng)
    assert [len(per[0][key]) for key in ("u", "x", "pi", "lam", "t")] == [N, N + 1, N, N + 1, N + 1]
    for p in range(2):
        for key in flat:
            assert np.array_equal(np.concatenate(per[p][key]), flat[key][p]), key
        assert per[p]["lam"][4].shape == (2 * P["nb"][4] + 2 * ng[4],)


def test_flatten_rejects_mismatched_sizes():
    with pytest.raises(ValueError):
        flatten_problems([IO.random_iface_problem(*F, seed=1), IO.random_iface_problem(*V, seed=1)])


def test_layout_equals_the_written_out_sums():
    N, nx, nu, bu, bx, ng = V
    nb = IO.random_iface_problem(*V, seed=1)["nb"]
    assert nb == [2, 4, 3, 4, 4, 2]
    lay = ocp_dense_layout(N, nx, nu, nb, ng)
    sz, off = lay["sizes"], lay["offsets"]
    nuN = nu + [0]
    want = dict(A=sum(nx[k + 1] * nx[k] for k in range(N)), B=sum(nx[k + 1] * nu[k] for k in range(N)),
                b=sum(nx[1:]), Q=sum(v * v for v in nx), S=sum(nu[k] * nx[k] for k in range(N)),
                R=sum(v * v for v in nu), q=sum(nx), r=sum(nu), lb=sum(nb), ub=sum(nb),
                C=sum(ng[k] * nx[k] for k in range(N + 1)), D=sum(ng[k] * nuN[k] for k in range(N + 1)),
                lg=sum(ng), ug=sum(ng), u=sum(nu), x=sum(nx), pi=sum(nx[1:]), lam=2 * sum(nb) + 2 * sum(ng),
                t=2 * sum(nb) + 2 * sum(ng))
    assert sz == want
    # A: 3x0, 3x3, 5x3, 5x5, 4x5; C: ng = 0,0,2,0,3,2 rows of nx = 0,3,3,5,5,4 columns
    assert list(off["A"]) == [0, 0, 9, 24, 49, 69] and sz["A"] == 69
    assert list(off["C"]) == [0, 0, 0, 6, 6, 21] and sz["C"] == 29
    assert list(off["D"]) == [0, 0, 0, 2, 2, 11] and sz["D"] == 11
    assert list(off["lam"]) == [0, 4, 12, 22, 30, 44] and sz["lam"] == 52
    assert list(off["u"]) == list(off["r"]) and list(off["x"]) == list(off["q"]) and list(off["pi"]) == list(off["b"])


def test_wide_cases_sit_on_the_tile_edge():
    """What H, E and B are in the table for, read off the problems IO.random_iface_problem makes of them: the stage
    sizes at which a 16-double ux / pi slot or a 32-double lam / t slot is full."""
    r4 = lambda n: (n + 3) // 4 * 4
    slots = lambda P: [2 * r4(b) + 2 * r4(g) for b, g in zip(P["nb"], P["ng"])]
    Ph, Pe, Pb = (IO.random_iface_problem(*c, seed=1) for c in (H, E, B))
    # H: (nu, nx) = (4, 12) on every inner stage, an empty x_0, nb = 8 on the inner stages
    assert Ph["nx"][0] == 0 and all((Ph["nu"][k], Ph["nx"][k]) == (4, 12) for k in range(1, 5))
    assert Ph["nb"] == [4, 8, 8, 8, 8, 4] and not any(Ph["ng"])
    # E: every stage fills the 32 slots, in the splits 4 + 12, 8 + 8 (both padded), 8 + 8, 8 + 8, 0 + 16
    assert slots(Pe) == [32] * 5
    assert list(zip(Pe["nb"], Pe["ng"])) == [(4, 12), (5, 7), (8, 8), (8, 8), (0, 16)]
    assert [u + x for u, x in zip(Pe["nu"], Pe["nx"])] == [8, 16, 16, 16, 16] and Pe["nu"][2] == 0
    assert Pe["nx"][0] > 0 and Pe["ng"][0] > 0          # a variable x_0 under general constraints
    assert list(Pe["hidxb"][3]) == list(range(8))       # stage 3: every box on an input
    # B: every variable of stages 1 and 2 boxed, lam / t full; stage 0 with nx 4 and nb 12
    assert Pb["nb"] == [12, 16, 16, 8] and slots(Pb)[1:3] == [32, 32] and (Pb["nu"][1], Pb["nx"][1]) == (8, 8)
    lay = ocp_dense_layout(Pe["N"], Pe["nx"], Pe["nu"], Pe["nb"], Pe["ng"])
    assert lay["sizes"]["lam"] == 2 * sum(Pe["nb"]) + 2 * sum(Pe["ng"]) == 152
    assert lay["sizes"]["C"] == 12 * 4 + 7 * 12 + 8 * 16 + 8 * 8 + 16 * 16
    assert lay["sizes"]["D"] == 12 * 4 + 7 * 4 + 0 + 64


def test_header_declares_and_export_map_lists_the_new_functions():
    header = open(os.path.join(ROOT, "include", "hpmpc_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "typedef struct hpmpc_mi355x_ocp_plan hpmpc_mi355x_ocp_plan;" in header
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
    m = re.search(r"\bint\s+hpmpc_mi355x_ocp_ipm_batch\s*\(([^;]*)\)\s*;", header)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    # hpmpc_mi355x_ipm_batch's list plus DCt, minus the layout
    assert len(args) == 23 and args[0].startswith("const hpmpc_mi355x_ocp_plan") and args[-1] == "void *stream"
    assert "const double *DCt" in args and not any("layout" in a for a in args)
    emap = open(os.path.join(ROOT, "hpmpc_amd", "csrc", "exports.map")).read()
    emap = re.sub(r"/\*.*?\*/", "", emap, flags=re.S)
    glob = re.search(r"global:(.*?)local:", emap, flags=re.S).group(1)
    patterns = [p.strip() for p in glob.split(";") if p.strip()]
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name
    # the build compiles the new files
    from hpmpc_amd.build import HEADERS, SOURCES

    assert "hk_ocp.hip" in SOURCES and "hpmpc_capi_ocp.cpp" in SOURCES and "hk_ocp_args.h" in HEADERS

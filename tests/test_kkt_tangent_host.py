"""Host-side checks (no GPU) of the batched KKT tangent solve: the three new entry points are declared in the header,
bound in hpmpc_amd.bindings and exported by the built library; tangent_set_arrays is the direction twin of
kkt_set_arrays; the new kernel's sources are part of the build; and the reference preconditions the GPU tests rely
on (kkt_tangent_cases.TanRefs.usable) hold on the CPU oracle's two builds."""
import os

import numpy as np
import pytest

import kkt_tangent_cases as TC
from hpmpc_amd import bindings, build, ocp_batch
from ocp_batch_cases import problems
from test_bindings_host import header_signatures

NEW = ("hpmpc_mi355x_kkt_tangent_batch", "hpmpc_mi355x_ocp_tangent_batch", "hpmpc_mi355x_ocp_unpack_sets")


def test_entry_points_are_declared_and_bound():
    want = header_signatures()
    for name in NEW:
        assert name in want, name
        assert name in bindings.SIGNATURES, name
        assert bindings.SIGNATURES[name][0] is want[name][0] and list(bindings.SIGNATURES[name][1]) == want[name][1]
    # the core call has the re-solve's argument list, the dense one an OCP plan and a direction struct in front
    assert want[NEW[0]] == want["hpmpc_mi355x_kkt_new_rhs_batch"]
    assert len(want[NEW[1]][1]) == 18 and len(want[NEW[2]][1]) == 16
    assert "hk_tan.hip" in build.SOURCES and "hpmpc_capi_kkt.cpp" in build.SOURCES  # the tangent's host entry points
    assert {"hk_tan_args.h", "hk_tan_body.h", "hk_ocp_plan.h", "hk_ocp_place.h", "hk_kkt_launch.h"} <= set(build.HEADERS)
    assert "hk_tan.hip" in build.SRC_FLAGS


def test_built_library_exports_them():
    if not os.path.exists(bindings.LIBPATH):
        build.build_hip()
    L = bindings.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is bindings.SIGNATURES[name][0] and list(fn.argtypes) == list(bindings.SIGNATURES[name][1])
    # the refusals that need no device: no plan
    assert L.hpmpc_mi355x_kkt_tangent_batch(None, None, 1, 0, 1, 1, *([None] * 12), 1, None) == -10
    assert L.hpmpc_mi355x_ocp_tangent_batch(None, None, 1, 0, 1, 1, *([None] * 10), 1, None) == -10
    assert L.hpmpc_mi355x_ocp_unpack_sets(None, 1, 0, 1, 1, *([None] * 11)) == -10
    assert L.hpmpc_mi355x_last_error() == -10


@pytest.mark.parametrize("case", ["V", "S", "H", "E", "B"])
def test_tangent_set_arrays_is_the_difference_of_kkt_set_arrays(case):
    Ps = problems(case, (0, 1, 2))
    rng = np.random.default_rng(3)
    # exactly representable: the data rounded to 2^-20, deltas multiples of 2^-10 -- sums and differences are exact
    grid = lambda v, s: np.round(np.asarray(v) * s) / s
    base, deltas = [], []
    for P in Ps:
        Q = dict(P)
        D = {k: P[k] for k in ("N", "nx", "nu", "nb", "ng")}
        for key in ocp_batch.VEC_KEYS:
            Q[key] = [grid(v, 2.0 ** 20) for v in P[key]]
            D[key] = [grid(rng.standard_normal(np.shape(v)), 2.0 ** 10) for v in P[key]]
        base.append(Q)
        deltas.append(D)
    moved = [TC.shifted(Q, D) for Q, D in zip(base, deltas)]
    for got, hi, lo in zip(ocp_batch.tangent_set_arrays(deltas), ocp_batch.kkt_set_arrays(moved),
                           ocp_batch.kkt_set_arrays(base)):
        assert got.shape == hi.shape and np.any(got != 0.0)
        assert np.array_equal((hi - lo).view(np.int64), got.view(np.int64))
    # a missing key is a zero direction
    only_b = [{k: D[k] for k in ("N", "nx", "nu", "nb", "ng", "b")} for D in deltas]
    db, dq, dd = ocp_batch.tangent_set_arrays(only_b)
    assert np.array_equal(db, ocp_batch.tangent_set_arrays(deltas)[0]) and not dq.any() and not dd.any()


def test_x0_directions_are_the_columns():
    rng = np.random.default_rng(4)
    A0, S0 = rng.standard_normal((2, 8, 3)), rng.standard_normal((2, 3, 3))
    d = ocp_batch.x0_directions(A0, S0)
    assert d["b"].shape == (2, 3, 8) and d["r"].shape == (2, 3, 3)
    for i in range(3):
        assert np.array_equal(d["b"][:, i], A0[:, :, i]) and np.array_equal(d["r"][:, i], S0[:, :, i])
    assert set(ocp_batch.x0_directions(A0[0])) == {"b"}
    with pytest.raises(ValueError):
        ocp_batch.x0_directions(A0, S0[:, :, :2])


@pytest.mark.parametrize("case", TC.CASES)
def test_reference_preconditions(oracle, case):
    """Measured on liboracle.so / liboracle_fma.so: left out only F seed 2 (ret 1); build spread <= 6.9e-13 and
    affinity defect <= 1.3e-12 (both gated at TOL_IPM / 4 = 2.5e-11); problems with max |dlam_ref| >= 1e-2: V 10/10,
    V0 10/10, F 9/9, S 8/10.  H, E, B (the wide cases): none left out, spread <= 8.0e-13, defect <= 8.3e-13, 10/10
    each."""
    refs = TC.TanRefs(oracle)
    rows = refs.measure(case)
    print(case, [(r["seed"], r["ret"], r.get("spread"), r.get("affinity"), r.get("dlam")) for r in rows])
    used = refs.usable(case)
    assert len(used) >= 9
    if case != "F":
        assert used == list(TC.SEEDS)

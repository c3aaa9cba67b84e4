"""Host-side checks (no GPU) of the OCP matrix directions: the two new entry points are declared in the header, bound in
hpmpc_amd.bindings and exported by the built library; the new kernel's sources are part of the build; the reference
preconditions the GPU tests rely on (kkt_matdir_cases.DirRefs.usable) hold on the CPU oracle's two builds; the five
seed-row formulas of include/hpmpc_mi355x.h, restated in numpy, reproduce the oracle's residual difference dF (signs
and the sym convention, with no GPU); and <adj, dF> equals <formulas of the matrix gradients, dtheta> for dQ and dR
that are not symmetric."""
import os

import numpy as np
import pytest

import kkt_matdir_cases as DC
import kkt_matgrad_cases as MC
from hpmpc_amd import bindings, build, ocp_batch
from hpmpc_amd.ocp_batch import MAT_KEYS, VEC_KEYS
from test_bindings_host import header_signatures

NEW = ("hpmpc_mi355x_ocp_matrix_dirs_batch", "hpmpc_mi355x_ocp_tangent_data_batch")


@pytest.fixture(scope="module")
def refs(oracle):
    return DC.shared(oracle)


def test_entry_points_are_declared_and_bound():
    want = header_signatures()
    for name in NEW:
        assert name in want, name
        assert name in bindings.SIGNATURES, name
        assert bindings.SIGNATURES[name][0] is want[name][0] and list(bindings.SIGNATURES[name][1]) == want[name][1]
    assert len(want[NEW[0]][1]) == 13 and len(want[NEW[1]][1]) == 21
    assert "hk_matdir.hip" in build.SOURCES and "hk_matdir_args.h" in build.HEADERS
    for name in ("hk_matdir.hip", "hk_matdir_args.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    for name in ("matrix_directions", "tangent_data", "direction_buffers"):
        assert callable(getattr(ocp_batch.OcpBatchSolver, name)), name


def test_built_library_exports_them():
    if not os.path.exists(bindings.LIBPATH):
        build.build_hip()
    L = bindings.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is bindings.SIGNATURES[name][0] and list(fn.argtypes) == list(bindings.SIGNATURES[name][1])
    # the refusals that need no device: no plan
    assert L.hpmpc_mi355x_ocp_matrix_dirs_batch(None, None, 1, 0, 1, 1, *([None] * 7)) == -10
    assert L.hpmpc_mi355x_last_error() == -10
    assert L.hpmpc_mi355x_ocp_tangent_data_batch(None, None, 1, 0, 1, 1, *([None] * 13), 1, None) == -10
    assert L.hpmpc_mi355x_last_error() == -10


@pytest.mark.parametrize("case", DC.CASES)
def test_reference_preconditions(refs, case):
    """Measured on liboracle.so / liboracle_fma.so: the seeds are TanRefs.usable's (only F seed 2 left out); build spread
    of the reference tangents <= 2.1e-12 (gated at TOL_IPM / 4 = 2.5e-11) with SCALE = 1; on V every problem has max
    |dlam_ref| >= 0.2 and the C / D direction alone moves the residuals by >= 0.17 / >= 0.08.  H, E, B: none left out,
    spread <= 1.3e-11 / 2.6e-12 / 5.1e-13; on E |dlam_ref| >= 1.1 and the C / D moves are >= 0.58 / >= 0.21."""
    rows = refs.measure(case)
    print(case, [(r["seed"], r["spread"], r["dlam"], r["dFC"], r["dFD"]) for r in rows])
    used = refs.usable(case)
    assert used == refs.tan.usable(case) and len(used) >= 9


@pytest.mark.parametrize("case", DC.CASES)
def test_formulas_reproduce_the_oracles_seed(refs, case):
    """The five formulas at the oracle IPM's final iterate against the oracle's residual difference, per key at
    1e-12 max(1, sum |terms|): both are the same bilinear form, dF a difference of two residual evaluations."""
    for seed in refs.usable(case):
        P, z = refs.ipm(case, seed)[:2]
        dF = refs.seed(case, seed)[0]
        got, mag = DC.formulas(P, z, refs.dtheta(case, seed))
        for key in VEC_KEYS:
            assert got[key].shape == dF[key].shape, (case, key)
            err = float(np.max(np.abs(got[key] - dF[key]), initial=0.0))
            print(case, seed, key, err, mag[key])
            assert err <= 1e-12 * max(1.0, mag[key]), (case, seed, key, err, mag[key])
        assert max(mag[k] for k in ("b", "q")) > 1e-3
        # one matrix alone: a missing key contributes no term
        for only in ("A", "C"):
            one, _ = DC.formulas(P, z, {only: refs.dtheta(case, seed)[only]})
            dF1 = refs.seed(case, seed, (only,))[0]
            for key in VEC_KEYS:
                assert np.max(np.abs(one[key] - dF1[key]), initial=0.0) <= 1e-12 * max(1.0, mag[key]), (case, only, key)


@pytest.mark.parametrize("case", DC.CASES)
def test_pairing_with_the_matrix_gradients(refs, case):
    """<adj, dF> == <MC.formulas(P, z, adj), dtheta> for dQ, dR NOT symmetric: gQ and gR are symmetric, so they see only
    the symmetric parts that dF was evaluated with.  Same bilinear form on both sides; bound 1e-12 max(1, S) with S the
    absolute sum, as in test_kkt_matgrad_host.test_dot_product_identity."""
    for seed in refs.usable(case)[:3]:
        P, z = refs.ipm(case, seed)[:2]
        adj = refs.adj.adjoint(case, seed)[0]
        dth = refs.dtheta(case, seed)
        assert any(not np.array_equal(M, M.T) for M in dth["Q"] if M.size > 1)
        lhs = MC.dot(adj, refs.seed(case, seed)[0], VEC_KEYS)
        G = MC.formulas(P, z, adj)
        rhs = sum(float(np.sum(g * d)) for key in MAT_KEYS for g, d in zip(G[key], dth[key]))
        S = sum(float(np.sum(np.abs(g * d))) for key in MAT_KEYS for g, d in zip(G[key], dth[key]))
        print(case, seed, lhs, abs(lhs - rhs) / max(1.0, S))
        assert S > 1e-3 and abs(lhs - rhs) <= 1e-12 * max(1.0, S), (case, seed, lhs, rhs, S)

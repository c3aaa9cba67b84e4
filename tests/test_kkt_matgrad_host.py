"""Host-side checks (no GPU) of the OCP matrix gradients: the two new entry points are declared in the header, bound in
hpmpc_amd.bindings and exported by the built library; the new kernel's sources are part of the build; the reference
preconditions the GPU tests rely on (kkt_matgrad_cases.MatRefs.usable) hold on the CPU oracle's two builds; the seven
outer-product formulas of include/hpmpc_mi355x.h, restated in numpy, reproduce the reference (which evaluates the
oracle's residuals element by element and uses no formula); and <G, dtheta> equals g' T_ref (res(theta + dtheta) -
res(theta)) for random matrix perturbations."""
import os

import numpy as np
import pytest

import kkt_matgrad_cases as MC
from helpers import TOL_IPM
from hpmpc_amd import bindings, build, ocp_batch
from hpmpc_amd.ocp_batch import MAT_KEYS, VEC_KEYS
from test_bindings_host import header_signatures

NEW = ("hpmpc_mi355x_ocp_matrix_grads_batch", "hpmpc_mi355x_ocp_adjoint_data_batch")


@pytest.fixture(scope="module")
def refs(oracle):
    return MC.shared(oracle)


def test_entry_points_are_declared_and_bound():
    want = header_signatures()
    for name in NEW:
        assert name in want, name
        assert name in bindings.SIGNATURES, name
        assert bindings.SIGNATURES[name][0] is want[name][0] and list(bindings.SIGNATURES[name][1]) == want[name][1]
    assert len(want[NEW[0]][1]) == 13 and len(want[NEW[1]][1]) == 20
    assert "hk_matgrad.hip" in build.SOURCES and "hk_matgrad_args.h" in build.HEADERS
    for name in ("hk_matgrad.hip", "hk_matgrad_args.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name
    assert set(MAT_KEYS) | set(VEC_KEYS) == set(ocp_batch.KEYS) and not set(MAT_KEYS) & set(VEC_KEYS)
    assert ocp_batch._OcpGrads._fields_[0][1]._length_ == len(ocp_batch.KEYS)


def test_built_library_exports_them():
    if not os.path.exists(bindings.LIBPATH):
        build.build_hip()
    L = bindings.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is bindings.SIGNATURES[name][0] and list(fn.argtypes) == list(bindings.SIGNATURES[name][1])
    # the refusals that need no device: no plan
    assert L.hpmpc_mi355x_ocp_matrix_grads_batch(None, 1, 0, 1, 1, *([None] * 8)) == -10
    assert L.hpmpc_mi355x_last_error() == -10
    assert L.hpmpc_mi355x_ocp_adjoint_data_batch(None, 1, 0, 1, 1, *([None] * 15)) == -10
    assert L.hpmpc_mi355x_last_error() == -10


@pytest.mark.parametrize("case", MC.CASES)
def test_reference_preconditions(refs, case):
    """Measured on liboracle.so / liboracle_fma.so: the seeds are AdjRefs.usable's (only F seed 2 left out); build
    spread of the reference gradients <= 1.4e-12 (gated at TOL_IPM / 4 = 2.5e-11); on V every problem has max |gC| >=
    0.19 and max |gD| >= 0.057.  H, E, B: the first three seeds (kkt_matgrad_cases, Cost), spread <= 3.1e-13 / 6.5e-12 /
    9.5e-15; on E max |gC| >= 1.35 and max |gD| >= 0.45."""
    rows = refs.measure(case)
    print(case, [(r["seed"], r["nel"], r["spread"], r["gC"], r["gD"]) for r in rows])
    used = refs.usable(case)
    full = refs.adj.usable(case)
    assert full == refs.adj.tan.usable(case) and len(full) >= 9
    assert used == (full[:MC.N_WIDE] if case in MC.WIDE else full)


@pytest.mark.parametrize("case", MC.CASES)
def test_formulas_reproduce_the_reference(refs, case):
    """The outer products at the oracle IPM's final iterate, with the reference adjoint T_ref' g as (bbar, qbar,
    dbar)."""
    for seed in refs.usable(case):
        P, z = refs.ipm(case, seed)[:2]
        ref = refs.gradients(case, seed)[0]
        got = MC.formulas(P, z, refs.adj.adjoint(case, seed)[0])
        for key in MAT_KEYS:
            assert [np.shape(M) for M in got[key]] == [np.shape(M) for M in ref[key]], (case, key)
        err = MC.mat_err(got, ref)
        print(case, seed, err)
        assert err <= TOL_IPM / 4, (case, seed, err)
        for key in MC.SYM_KEYS:
            assert all(np.array_equal(M, M.T) for M in got[key])


@pytest.mark.parametrize("case", MC.CASES)
def test_dot_product_identity(refs, case):
    """<G, dtheta> == g' T_ref (res(theta + dtheta) - res(theta)) for a random dtheta over all seven matrices at once
    (dQ, dR symmetric), with the IPM's final iterate and with the base re-solve's output as z.  Both sides are the same
    bilinear form in exact arithmetic: each is a sum of at most ~1e3 products and dF a difference of two residual
    evaluations, so they agree to a few hundred roundings of the absolute sum S = sum |G| |dtheta|; the bound is 1e-12
    max(1, S) (2^-53 x 1e3 terms x 10)."""
    for seed in refs.usable(case)[:3]:
        P, ipm0 = refs.ipm(case, seed)[:2]
        api = refs.apis[0]
        adj = refs.adj.adjoint(case, seed)[0]
        resolved = refs.adj.tan.resolve(case, seed, None, "base")[1]
        rng = np.random.default_rng(7 + seed)
        P2, dth = dict(P), {}
        for key in MAT_KEYS:
            dth[key] = [rng.standard_normal(np.shape(M)) for M in P[key]]
            if key in MC.SYM_KEYS:
                dth[key] = [0.5 * (M + M.T) for M in dth[key]]
            P2[key] = [np.asarray(M) + d for M, d in zip(P[key], dth[key])]
        for z in (ipm0, resolved):
            base, mv = MC.residuals_at(api, P, z), MC.residuals_at(api, P2, z)
            rhs = MC.dot(adj, {c: mv[c] - base[c] for c in VEC_KEYS}, VEC_KEYS)
            G = MC.formulas(P, z, adj)
            lhs = sum(float(np.sum(g * d)) for key in MAT_KEYS for g, d in zip(G[key], dth[key]))
            S = sum(float(np.sum(np.abs(g * d))) for key in MAT_KEYS for g, d in zip(G[key], dth[key]))
            print(case, seed, lhs, abs(lhs - rhs) / max(1.0, S))
            assert S > 1e-3 and abs(lhs - rhs) <= 1e-12 * max(1.0, S), (case, seed, lhs, rhs, S)

"""Host-side checks (no GPU) of the batched KKT adjoint solve: the two new entry points are declared in the header,
bound in hpmpc_amd.bindings and exported by the built library; the new kernel's sources are part of the build;
adjoint_set_arrays is the transpose of the dense outputs' placement; the reference preconditions the GPU tests rely on
(kkt_adjoint_cases.AdjRefs.usable) hold on the CPU oracle's two builds; and the three-step adjoint formula of
csrc/hk_adj_body.h, restated in numpy, reproduces T_ref' g."""
import os

import numpy as np
import pytest

import kkt_adjoint_cases as AC
import kkt_tangent_cases as TC
from helpers import TOL_IPM
from hpmpc_amd import bindings, build, ocp_batch
from ocp_batch_cases import problems
from test_bindings_host import header_signatures

NEW = ("hpmpc_mi355x_kkt_adjoint_batch", "hpmpc_mi355x_ocp_adjoint_batch")


@pytest.fixture(scope="module")
def refs(oracle):
    return AC.AdjRefs(oracle)


def test_entry_points_are_declared_and_bound():
    want = header_signatures()
    for name in NEW:
        assert name in want, name
        assert name in bindings.SIGNATURES, name
        assert bindings.SIGNATURES[name][0] is want[name][0] and list(bindings.SIGNATURES[name][1]) == want[name][1]
    assert len(want[NEW[0]][1]) == 19 and len(want[NEW[1]][1]) == 23
    assert "hk_adj.hip" in build.SOURCES and "hpmpc_capi_kkt.cpp" in build.SOURCES
    assert {"hk_adj_args.h", "hk_adj_body.h", "hk_ocp_place.h", "hk_kkt_launch.h"} <= set(build.HEADERS)
    assert build.SRC_FLAGS["hk_adj.hip"] == build.SRC_FLAGS["hk_tan.hip"]
    for name in ("hk_adj.hip", "hk_adj_args.h", "hk_adj_body.h"):
        assert os.path.exists(os.path.join(build.CSRC, name)), name


def test_built_library_exports_them():
    if not os.path.exists(bindings.LIBPATH):
        build.build_hip()
    L = bindings.lib()
    for name in NEW:
        fn = getattr(L, name)
        assert fn.restype is bindings.SIGNATURES[name][0] and list(fn.argtypes) == list(bindings.SIGNATURES[name][1])
    # the refusals that need no device: no plan
    assert L.hpmpc_mi355x_kkt_adjoint_batch(None, None, 1, 0, 1, 1, *([None] * 13)) == -10
    assert L.hpmpc_mi355x_last_error() == -10
    assert L.hpmpc_mi355x_ocp_adjoint_batch(None, 1, 0, 1, 1, *([None] * 18)) == -10
    assert L.hpmpc_mi355x_last_error() == -10


@pytest.mark.parametrize("case", ["V", "S", "H", "E", "B"])
def test_adjoint_set_arrays_is_the_transpose_of_the_dense_placement(case):
    """<dense_of(P, it), g> == <it, adjoint_set_arrays(g)> exactly, on integer-valued data (every sum is exact)."""
    rng = np.random.default_rng(5)
    ints = lambda shape: rng.integers(-8, 9, size=shape).astype(np.float64)
    for P in problems(case, (0, 1)):
        N = P["N"]
        it = dict(ux=ints((N + 1, 16)), pi=ints((N + 1, 16)), lam=ints((N + 1, 32)), t=ints((N + 1, 32)))
        dense = TC.dense_of(P, it)
        g = {key: ints(dense[key].shape) for key in TC.OUT_KEYS}
        gux, gpi, glam, gt = (x[0] for x in ocp_batch.adjoint_set_arrays([AC.per_stage(P, g)]))
        lhs = sum(float(np.sum(dense[key] * g[key])) for key in TC.OUT_KEYS)
        rhs = float(np.sum(it["ux"] * gux) + np.sum(it["pi"] * gpi) + np.sum(it["lam"] * glam) + np.sum(it["t"] * gt))
        assert lhs == rhs and lhs != 0.0
        # every dense element lands in exactly one padded slot, unscaled
        for arrs, keys in (((gux,), ("u", "x")), ((gpi,), ("pi",)), ((glam,), ("lam",)), ((gt,), ("t",))):
            assert sum(float(np.abs(a).sum()) for a in arrs) == sum(float(np.abs(g[k]).sum()) for k in keys)
        # a missing key is zero
        only_u = {k: v for k, v in AC.per_stage(P, g).items() if k not in ("x", "pi", "lam", "t")}
        a = ocp_batch.adjoint_set_arrays([only_u])
        assert not a[1].any() and not a[2].any() and not a[3].any() and a[0].any()


@pytest.mark.parametrize("case", AC.CASES)
def test_reference_preconditions(refs, case):
    """Measured on liboracle.so / liboracle_fma.so: left out only F seed 2; 89 to 132 columns per problem; build
    spread of the reference adjoint <= 1.8e-12 (gated at TOL_IPM / 4 = 2.5e-11); problems with max |dbar_ref| >= 1e-2:
    V 10/10, V0 10/10, F 9/9, S 10/10.  H, E, B (the wide cases): 220 / 276 / 180 columns, spread <= 1.2e-11 / 1.7e-12
    / 5.4e-13, 10/10 each."""
    rows = refs.measure(case)
    print(case, [(r["seed"], r["ncol"], r["spread"], r["dbar"]) for r in rows])
    used = refs.usable(case)
    assert used == refs.tan.usable(case) and len(used) >= 9
    if case != "F":
        assert used == list(TC.SEEDS)


def _index_sets(P, sizes):
    """Positions of the lower / upper constraint slots: in the compact lam / t rows and in the lb+lg / ub+ug columns
    (both in the order: all boxes by stage, then all general constraints by stage)."""
    N, nb, ng = P["N"], P["nb"], P["ng"]
    row = {k: [] for k in AC.D_KEYS}
    o = 0
    for k in range(N + 1):
        for key, n in (("lb", nb[k]), ("ub", nb[k]), ("lg", ng[k]), ("ug", ng[k])):
            row[key] += list(range(o, o + n))
            o += n
    assert o == sizes["lam"]
    return np.array(row["lb"] + row["lg"], dtype=int), np.array(row["ub"] + row["ug"], dtype=int)


@pytest.mark.parametrize("case", ["V", "S", "B"])
def test_three_step_formula_reproduces_the_reference(refs, case):
    """h = gt - w glam, c = h_lo - h_up; (y_ux, y_pi) = S(gux + C' c, gpi); qbar = y_ux, bbar = y_pi, z = C y_ux,
    dbar_lo = -h_lo - w_lo z, dbar_up = h_up - w_up z -- with S, w and C all read off T_ref itself: S its (u, x, pi) x
    (r, q, b) block, w = -dlam / dt on each slot's own bound column, C from dt_lo = C dux over the (r, q, b) columns.

    Not run at H and E.  This restatement recovers w and C from T_ref by least squares, so T_ref's own rounding (the two
    builds differ by up to 1.2e-11 at H) enters twice and is multiplied by w.  Measured: every seed of V, S and B is
    under 7e-12, H has 2.0e-11 on seed 2 and 9.5e-11 on seed 5, E has 1.9e-11 on seed 4 and 4.3e-10 on seed 8 -- above
    this test's TOL_IPM / 4, while the reference adjoint T_ref' g that the GPU tests compare with spreads by at most
    1.2e-11 / 1.7e-12 between the builds at H / E (test_reference_preconditions).  The bound is kept and the two cases
    are left out, not the other way round: what fails there is this way of reading w off T_ref, not the reference."""
    for seed in refs.usable(case):
        P = refs.ipm(case, seed)[0]
        T = refs.matrix(case, seed)[0]
        s = refs.sizes(case, seed)
        ro, co = {}, {}
        o = 0
        for key in AC.OUT_KEYS:
            ro[key] = np.arange(o, o + s[key])
            o += s[key]
        o = 0
        for key in ocp_batch.VEC_KEYS:
            co[key] = np.arange(o, o + s[key])
            o += s[key]
        lo, up = _index_sets(P, s)
        ux_rows = np.concatenate([ro["u"], ro["x"]])
        rq_cols = np.concatenate([co["r"], co["q"]])
        lo_cols, up_cols = np.concatenate([co["lb"], co["lg"]]), np.concatenate([co["ub"], co["ug"]])
        rows_S, cols_S = np.concatenate([ux_rows, ro["pi"]]), np.concatenate([rq_cols, co["b"]])
        S = T[np.ix_(rows_S, cols_S)]
        # dlam = -w dt holds in every column: the least-squares ratio over a slot's whole row pair
        ratio = lambda rows: -np.sum(T[ro["lam"][rows]] * T[ro["t"][rows]], axis=1) / np.sum(T[ro["t"][rows]] ** 2, axis=1)
        w_lo, w_up = ratio(lo), ratio(up)
        # dt_lo + dd_lo = C dux holds in every column
        E = np.zeros((len(lo), T.shape[1]))
        E[np.arange(len(lo)), lo_cols] = 1.0
        Cm = np.linalg.lstsq(T[ux_rows].T, (T[ro["t"][lo]] + E).T, rcond=None)[0].T
        g, gd = refs.cotangent(case, seed)
        h_lo = gd["t"][lo] - w_lo * gd["lam"][lo]
        h_up = gd["t"][up] - w_up * gd["lam"][up]
        c = h_lo - h_up
        rhs = np.concatenate([np.concatenate([gd["u"], gd["x"]]) + Cm.T @ c, gd["pi"]])
        y = S @ rhs
        y_ux, y_pi = y[:len(ux_rows)], y[len(ux_rows):]
        # z = C y_ux = (C S) rhs, and C S is T_ref's own dt rows over the (r, q, b) columns: dt_lo = C dux for the lower
        # slots, dt_up = -C dux for the upper ones, each slot from its own row.  Forming C (S rhs) from the dense S
        # instead cancels to rounding on an active constraint, where w (up to 7.6e3 here) multiplies it
        z_lo = T[np.ix_(ro["t"][lo], cols_S)] @ rhs
        z_up = -T[np.ix_(ro["t"][up], cols_S)] @ rhs
        d_lo, d_up = -h_lo - w_lo * z_lo, h_up - w_up * z_up
        nlb, nub = s["lb"], s["ub"]
        got = dict(r=y_ux[:s["u"]], q=y_ux[s["u"]:], b=y_pi, lb=d_lo[:nlb], lg=d_lo[nlb:], ub=d_up[:nub], ug=d_up[nub:])
        ref = refs.adjoint(case, seed, g)[0]
        err = AC.grad_err(got, ref)
        print(case, seed, err)
        assert err <= TOL_IPM / 4, (case, seed, err)

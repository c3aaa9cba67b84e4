"""Shared by tests/test_kkt_adjoint_host.py (CPU) and tests/test_gpu_kkt_adjoint.py: the reference adjoints of the
batched KKT adjoint solve and the preconditions every test on them asserts.  Oracle only; nothing here loads the HIP
library.

Problems, IPM settings and re-solves are kkt_tangent_cases' (TanRefs).  For a usable problem the reference tangent
MATRIX T_ref has one column per element of b, q, r, lb, ub, lg, ug -- TanRefs.tangent_of on that element's unit
direction, a difference of two oracle re-solves -- and one row per element of the dense outputs u, x, pi, lam, t.  The
reference adjoint of a cotangent g (rows' order) is T_ref' g, split by column into the dense gradients.  The cotangent
of a problem is default_rng(100 + seed).standard_normal over the concatenated (u, x, pi, lam, t).

Preconditions (`usable`):
  1. the problems used are exactly TanRefs.usable(case): at most 1 of 10 left out per case;
  2. the reference adjoints of the two oracle builds differ by at most TOL_IPM / 4;
  3. every used problem has max |dbar_ref| >= 1e-2 over lb, ub, lg, ug (the constraint half is exercised).
Gate of a comparison against the reference (the GATES rule): max(TOL_IPM, 4 x the two builds' spread on that problem
and cotangent), relative to max(1, |ref|).  No gate comes from the product's output.

Measured at the wide cases H, E, B (all ten seeds used; 220 / 276 / 180 columns per problem): worst build spread of
the reference adjoint H 1.2e-11, E 1.7e-12, B 5.4e-13; max |dbar_ref| >= 5.5 / 4.1 / 3.6 on every problem.  H leaves a
factor of two under TOL_IPM / 4.
"""
import numpy as np

import kkt_tangent_cases as TC
from helpers import TOL_IPM
from hpmpc_amd.ocp_batch import VEC_KEYS

CASES = TC.CASES
OUT_KEYS = TC.OUT_KEYS  # the rows of T_ref: u, x, pi, lam, t
D_KEYS = ("lb", "ub", "lg", "ug")
DBAR_ACTIVE = 1e-2
SIZE_KEYS = ("N", "nx", "nu", "nb", "ng")


def columns(P):
    """The columns of T_ref: (key, stage block, element) over b, q, r, lb, ub, lg, ug in the dense arrays' order."""
    return [(key, k, i) for key in VEC_KEYS for k, blk in enumerate(P[key]) for i in range(np.size(blk))]


def unit_delta(P, col):
    key, k, i = col
    D = {s: P[s] for s in SIZE_KEYS}
    for name in VEC_KEYS:
        D[name] = [np.zeros(np.shape(v)) for v in P[name]]
    D[key][k][i] = 1.0
    return D


def cat(dense, keys):
    return np.concatenate([np.asarray(dense[key], dtype=np.float64).ravel() for key in keys] + [np.zeros(0)])


def split(vec, sizes, keys):
    """A concatenated vector -> {key: its part}, with sizes[key] elements each."""
    out, o = {}, 0
    for key in keys:
        out[key] = np.asarray(vec[o:o + sizes[key]], dtype=np.float64).copy()
        o += sizes[key]
    assert o == len(vec)
    return out


def rel(a, b):
    return TC.rel(a, b)


def grad_err(got, ref):
    """max over b, q, r, lb, ub, lg, ug of |got - ref| / max(1, |ref|)"""
    return max(rel(got[key], ref[key]) for key in VEC_KEYS)


def per_stage(P, dense, keys=OUT_KEYS):
    """Dense vectors of one set -> interface-form per-stage lists (the input of adjoint_set_arrays)."""
    from hpmpc_amd.ocp_batch import unflatten_problems

    flat = {key: np.asarray(dense[key])[None] for key in keys}
    out = unflatten_problems(flat, P["N"], P["nx"], P["nu"], P["nb"], P["ng"], keys=list(keys))[0]
    out.update({s: P[s] for s in SIZE_KEYS})
    return out


class AdjRefs:
    """Reference tangent matrices and adjoints, computed once per key and shared (never modified)."""

    def __init__(self, oracle):
        self.tan = TC.TanRefs(oracle)
        self.cache = {}

    def ipm(self, case, seed):
        return self.tan.ipm(case, seed)

    def sizes(self, case, seed):
        """{key: elements} of the rows' (u, x, pi, lam, t) and the columns' (b, q, r, lb, ub, lg, ug) dense vectors"""
        P = self.ipm(case, seed)[0]
        ref = self.matrix(case, seed)[2]
        out = {key: int(sum(np.size(v) for v in P[key])) for key in VEC_KEYS}
        out.update({key: ref[key].size for key in OUT_KEYS})
        return out

    def matrix(self, case, seed):
        """(T_ref of liboracle.so, of liboracle_fma.so, the first column as a dense dict for the row sizes)"""
        key = ("T", case, seed)
        if key not in self.cache:
            P = self.ipm(case, seed)[0]
            cols = [self.tan.tangent_of(case, seed, unit_delta(P, col), ("unit", col)) for col in columns(P)]
            T = tuple(np.stack([cat(c[b], OUT_KEYS) for c in cols], axis=1) for b in (0, 1))
            self.cache[key] = T + (cols[0][0],)
        return self.cache[key]

    def cotangent(self, case, seed):
        """the problem's cotangent: (the vector in the rows' order, the dense dict u, x, pi, lam, t)"""
        T = self.matrix(case, seed)[0]
        g = np.random.default_rng(100 + seed).standard_normal(T.shape[0])
        s = self.sizes(case, seed)
        return g, split(g, s, OUT_KEYS)

    def adjoint(self, case, seed, g=None):
        """(reference adjoint of liboracle.so, of liboracle_fma.so): T_ref' g as dense dicts b, q, r, lb, ub, lg, ug"""
        g = self.cotangent(case, seed)[0] if g is None else g
        s = self.sizes(case, seed)
        return tuple(split(T.T @ g, s, VEC_KEYS) for T in self.matrix(case, seed)[:2])

    def gate(self, ref, alt):
        """the GATES rule from the two builds' spread on one problem and cotangent"""
        return max(TOL_IPM, 4 * grad_err(alt, ref))

    def measure(self, case):
        """Per usable seed: the two builds' spread on the reference adjoint and max |dbar_ref|."""
        rows = []
        for seed in self.tan.usable(case):
            ref, alt = self.adjoint(case, seed)
            rows.append(dict(seed=seed, spread=grad_err(alt, ref), ncol=self.matrix(case, seed)[0].shape[1],
                             dbar=float(np.max(np.abs(cat(ref, D_KEYS)), initial=0.0))))
        return rows

    def usable(self, case):
        """The seeds of the case a test may use, with the three preconditions asserted."""
        key = ("usable", case)
        if key not in self.cache:
            seeds = self.tan.usable(case)
            assert len(seeds) >= len(TC.SEEDS) - 1, (case, seeds)
            rows = self.measure(case)
            assert [r["seed"] for r in rows] == seeds
            for r in rows:
                assert r["spread"] <= TOL_IPM / 4, (case, r)
                assert r["dbar"] >= DBAR_ACTIVE, (case, r)
            self.cache[key] = seeds
        return self.cache[key]

"""Shared by tests/test_kkt_tangent_host.py (CPU) and tests/test_gpu_kkt_tangent.py: the reference tangents of the
batched KKT tangent solve and the preconditions every test on them asserts.  Oracle only; nothing here loads the HIP
library.

Inputs follow tests/test_gpu_kkt_batch.py: the cases V, V0, F, S, H, E, B of ocp_batch_cases with seeds 0..9, bounds
tightened x 0.25, solved with mu0 = 2, mu_tol = 1e-4, alpha_min = 1e-8, k_max = 50.  The direction of a problem P is
delta = IO.new_rhs(P, seed=6) - P (b, q, r and the four bound vectors) and the reference tangent is
orc_kkt(P + delta) - orc_kkt(P) on the oracle's own IPM work space: the re-solve is affine in these data, so the
difference IS the tangent, up to the rounding of the two re-solves.

Preconditions (`usable`):
  1. only problems whose oracle IPM returns ret != 0 are left out, at most 1 of 10 per case;
  2. the reference tangents of the two oracle builds (liboracle.so, liboracle_fma.so) differ by at most TOL_IPM / 4,
     and orc(P + 2 delta) - orc(P) equals twice the tangent to TOL_IPM / 4 (the reference itself is affine there);
  3. at least 8 used problems per case have max |dlam_ref| >= 1e-2 (the constraint half of the tangent is exercised).
Gate of a comparison against the reference (the GATES rule): max(TOL_IPM, 4 x the two builds' spread on that problem
and direction), relative to max(1, |ref|).  No gate comes from the product's output.

Measured on liboracle.so / liboracle_fma.so at the wide cases (H the compiled (4, 12) class, E the 16-wide tile edge
with general constraints, B every variable boxed), all ten seeds ret 0 with equal kk: worst build spread (affinity
defect) H 8.0e-13 (8.3e-13), E 4.8e-13 (7.6e-13), B 1.3e-13 (1.6e-13); max |dlam_ref| >= 1e-2 on 10 / 10 each.  The
re-solves of test_gpu_kkt_batch.py (right-hand-side seeds 6, 7, 8) spread by at most H 1.8e-12, E 4.3e-13, B 1.3e-13.
"""
import numpy as np

import test_gpu_kkt_batch as KB
from helpers import TOL_IPM
from hpmpc_amd.cabi import bq_from_qp
from hpmpc_amd.ocp_batch import VEC_KEYS, flatten_sets
from ocp_batch_cases import IO, K_MAX, compact, problems

CASES = ("V", "V0", "F", "S", "H", "E", "B")
SEEDS = range(10)
RSEED = 6
TIGHT = KB.TIGHT
MIN_ACTIVE = 8
DLAM_ACTIVE = 1e-2
ITER_KEYS = ("ux", "pi", "lam", "t")
OUT_KEYS = ("u", "x", "pi", "lam", "t")


def delta_of(P, P2):
    """P2 - P on the vector data, with the sizes of P: an interface-form delta."""
    D = {k: P[k] for k in ("N", "nx", "nu", "nb", "ng")}
    for key in VEC_KEYS:
        D[key] = [np.asarray(b) - np.asarray(a) for a, b in zip(P[key], P2[key])]
    return D


def shifted(P, D, scale=1.0):
    """P with its vector data moved by scale * D (matrices shared)."""
    Q = dict(P)
    for key in VEC_KEYS:
        if key in D:
            Q[key] = [np.asarray(a) + scale * np.asarray(d) for a, d in zip(P[key], D[key])]
    return Q


def scaled(D, scale):
    out = dict(D)
    for key in VEC_KEYS:
        if key in D:
            out[key] = [scale * np.asarray(d) for d in D[key]]
    return out


def iter_diff(a, b):
    """a - b for two oracle iterates (dicts of per-stage lists ux, pi, lam, t)."""
    return {key: [np.asarray(x) - np.asarray(y) for x, y in zip(a[key], b[key])] for key in ITER_KEYS}


def dense_of(P, it):
    """An iterate or tangent in the oracle's padded per-stage form (ux, pi, lam, t: lists, or arrays (N+1, 16 / 32))
    -> the dense OCP vectors u, x, pi, lam, t of one set: stage blocks concatenated, lam / t compact.  This is the
    numpy restatement of the placement hpmpc_mi355x_ocp_tangent_batch's epilogue and hpmpc_mi355x_ocp_unpack_sets do
    (without the equality-box fix)."""
    N, nx, nu = P["N"], P["nx"], P["nu"]
    cat = lambda v: np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in v] + [np.zeros(0)])
    return dict(u=cat([np.asarray(it["ux"][k])[:nu[k]] for k in range(N)]),
                x=cat([np.asarray(it["ux"][k])[nu[k]:nu[k] + nx[k]] for k in range(N + 1)]),
                pi=cat([np.asarray(it["pi"][k])[:nx[k + 1]] for k in range(N)]),
                lam=cat(compact(P, it["lam"])), t=cat(compact(P, it["t"])))


def rel(a, b):
    return KB._rel(a, b)


def dense_err(got, ref):
    """max over u, x, pi, lam, t of |got - ref| / max(1, |ref|)"""
    return max(rel(got[key], ref[key]) for key in OUT_KEYS)


def flat_dirs(deltas, ndir):
    """deltas[p][r] (interface-form deltas) -> {key: (nprob, ndir, size)} numpy arrays for OcpBatchSolver.tangent"""
    return flatten_sets(deltas, ndir, VEC_KEYS)


class TanRefs:
    """Oracle IPMs, re-solves and reference tangents, computed once per key and shared (never modified)."""

    def __init__(self, oracle):
        self.apis = (oracle, KB.fma_oracle())
        self.cache = {}

    def ipm(self, case, seed):
        """(P, the IPM result of liboracle.so, of liboracle_fma.so) on the tightened problem"""
        key = ("ipm", case, seed)
        if key not in self.cache:
            P = KB.tighten(problems(case, [seed])[0])
            self.cache[key] = (P,) + tuple(api.ipm(IO.to_qp(P), k_max=K_MAX, **TIGHT) for api in self.apis)
        return self.cache[key]

    def delta(self, case, seed, rseed=RSEED):
        P = self.ipm(case, seed)[0]
        return delta_of(P, IO.new_rhs(P, seed=rseed))

    def resolve(self, case, seed, D, tag):
        """(P + D, the re-solve of liboracle.so, of liboracle_fma.so); D = None: the base data.  tag: the cache key
        of the direction."""
        key = ("kkt", case, seed, tag)
        if key not in self.cache:
            P, *ipms = self.ipm(case, seed)
            P2 = P if D is None else shifted(P, D)
            qp2 = IO.to_qp(P2)
            b2, q2 = bq_from_qp(qp2)
            self.cache[key] = (P2,) + tuple(api.kkt_new_rhs(qp2.copy(), r["work"], b2, q2)
                                            for api, r in zip(self.apis, ipms))
        return self.cache[key]

    def tangent_of(self, case, seed, D, tag):
        """(reference tangent of liboracle.so, of liboracle_fma.so) for the delta D: orc(P + D) - orc(P), dense"""
        P = self.ipm(case, seed)[0]
        base = self.resolve(case, seed, None, "base")
        moved = self.resolve(case, seed, D, tag)
        return tuple(dense_of(P, iter_diff(m, b)) for m, b in zip(moved[1:], base[1:]))

    def tangent(self, case, seed, scale=1):
        """the reference tangents for scale * delta (delta = new_rhs(P, 6) - P), as differences of re-solves"""
        D = self.delta(case, seed)
        return self.tangent_of(case, seed, D if scale == 1 else scaled(D, scale), ("delta", scale))

    def gate(self, ref, alt):
        """the GATES rule from the two builds' spread on one problem and direction"""
        return max(TOL_IPM, 4 * dense_err(alt, ref))

    def measure(self, case):
        """Per seed of the case: ret, and for ret == 0 the build spread, the affinity defect and max |dlam_ref|."""
        rows = []
        for seed in SEEDS:
            P, r, rf = self.ipm(case, seed)
            row = dict(seed=seed, ret=r["ret"])
            if r["ret"] == 0:
                assert rf["kk"] == r["kk"] and rf["ret"] == 0, (case, seed)
                ref, alt = self.tangent(case, seed)
                two = self.tangent(case, seed, scale=2)[0]
                row.update(spread=dense_err(alt, ref),
                           affinity=dense_err(two, {k: 2 * v for k, v in ref.items()}),
                           dlam=float(np.max(np.abs(ref["lam"]), initial=0.0)))
            rows.append(row)
        return rows

    def usable(self, case):
        """The seeds of the case a test may use, with the three preconditions asserted."""
        key = ("usable", case)
        if key not in self.cache:
            rows = self.measure(case)
            used = [r for r in rows if r["ret"] == 0]  # ret != 0 is the only reason to leave a problem out
            assert len(used) >= len(SEEDS) - 1, (case, [r["seed"] for r in used])
            for r in used:
                assert r["spread"] <= TOL_IPM / 4, (case, r)
                assert r["affinity"] <= TOL_IPM / 4, (case, r)
            active = sum(r["dlam"] >= DLAM_ACTIVE for r in used)
            assert active >= MIN_ACTIVE, (case, active)
            self.cache[key] = [r["seed"] for r in used]
        return self.cache[key]

"""Shared by tests/test_kkt_matdir_host.py (CPU) and tests/test_gpu_kkt_matdir.py: the reference seed rows and tangents
for directions in all fourteen dense arrays, and the preconditions every test on them asserts.  Oracle only; nothing
here loads the HIP library.

Problems, IPM settings and re-solves are kkt_tangent_cases' (TanRefs), on the cases V, F and S.  For a usable seed the
matrix direction dtheta is SCALE * default_rng(11 + seed).standard_normal over the blocks of A, B, Q, S, R, C, D, with dQ
and dR NOT symmetrised.  The reference seed dF is residuals_at(api, P + dtheta_sym, z) - residuals_at(api, P, z) per
oracle build, at that build's own final IPM iterate z, where dtheta_sym replaces dQ and dR by their symmetric parts (the
oracle, like the kernels, reads one triangle of RSQrq): the oracle's residual routine evaluated twice, no formula of
ours.  The full direction adds the vector delta of kkt_tangent_cases (TanRefs.delta) and the reference tangent is
TanRefs.tangent_of on dF + delta: the difference of two oracle re-solves.  SCALE is 1: the spread condition holds for
the direction as drawn, so it was not scaled down.

Preconditions (`usable`):
  1. the seeds used are exactly TanRefs.usable(case): at most 1 of 10 left out, only for an oracle ret != 0;
  2. the reference tangents of the two oracle builds differ by at most TOL_IPM / 4 on every used problem;
  3. on every case with general constraints (ocp_batch_cases.GENERAL: V and E) at least 8 used problems have max
     |dlam_ref| >= 1e-2, and on every used problem the C and the D direction alone move the oracle's residuals (the
     constraint terms of dF are not zero).
Gate of a comparison against the reference (the GATES rule): max(TOL_IPM, 4 x the two builds' spread on that problem),
relative to max(1, |ref|).  No gate comes from the product's output.

Measured at the wide cases H, E, B (all ten seeds used): worst build spread of the reference tangent H 1.3e-11, E
2.6e-12, B 5.1e-13; on E every problem has max |dlam_ref| >= 1.1 and the C / D direction alone moves the residuals by
>= 0.58 / >= 0.21.  E's stage 3 holds 752 of the 768 direction doubles hk_ocp_matdir keeps in LDS.
"""
import numpy as np

import kkt_adjoint_cases as AC
import kkt_matgrad_cases as MC
import kkt_tangent_cases as TC
from helpers import TOL_IPM
from hpmpc_amd.ocp_batch import MAT_KEYS, VEC_KEYS
from ocp_batch_cases import GENERAL

CASES = ("V", "F", "S", "H", "E", "B")
SCALE = 1.0
MIN_ACTIVE = TC.MIN_ACTIVE
DLAM_ACTIVE = TC.DLAM_ACTIVE


def sym_part(dth):
    """dtheta with dQ and dR replaced by their symmetric parts"""
    out = dict(dth)
    for key in MC.SYM_KEYS:
        out[key] = [0.5 * (M + M.T) for M in dth[key]]
    return out


def moved_all(P, dth, keys=MAT_KEYS):
    """P with the blocks of `keys` moved by dth"""
    Q = dict(P)
    for key in keys:
        Q[key] = [np.asarray(M, dtype=np.float64) + d for M, d in zip(P[key], dth[key])]
    return Q


def add_delta(P, dF, D):
    """The dense seed dF {key: vector} plus the interface-form vector delta D -> an interface-form delta"""
    out = AC.per_stage(P, dF, keys=VEC_KEYS)
    for key in VEC_KEYS:
        out[key] = [np.asarray(a) + np.asarray(b) for a, b in zip(out[key], D[key])]
    return out


def formulas(P, z, dth, D=None):
    """The five seed-row formulas of include/hpmpc_mi355x.h in numpy: z the base iterate (padded ux, pi, lam per
    stage), dth the matrix directions {key: per-stage blocks} (a missing key: no term; dQ, dR any), D an interface-form
    vector delta or None -> the dense seed {b, q, r, lb, ub, lg, ug} of one set, and the sum of |terms| per key."""
    N, nx, nu, nb, ng = P["N"], P["nx"], P["nu"], P["nb"], P["ng"]
    blk = lambda key, k, shape: np.asarray(dth[key][k]) if key in dth and k < len(dth[key]) else np.zeros(shape)
    sym = lambda M: 0.5 * (M + M.T)
    out = {key: [] for key in VEC_KEYS}
    mag = {key: 0.0 for key in VEC_KEYS}

    def put(key, k, terms):
        v = sum(terms)
        if D is not None:
            v = v + np.asarray(D[key][k])
            terms = terms + [np.asarray(D[key][k])]
        out[key].append(v)
        mag[key] += float(sum(np.sum(np.abs(t)) for t in terms))

    for k in range(N + 1):
        nuk = nu[k] if k < N else 0
        nxk, ngk = nx[k], ng[k]
        pnb, png = (nb[k] + 3) // 4 * 4, (ng[k] + 3) // 4 * 4
        u, x = np.asarray(z["ux"][k])[:nuk], np.asarray(z["ux"][k])[nuk:nuk + nxk]
        lam = np.asarray(z["lam"][k])
        w = lam[2 * pnb + png:2 * pnb + png + ngk] - lam[2 * pnb:2 * pnb + ngk]
        dQ, dC = blk("Q", k, (nxk, nxk)), blk("C", k, (ngk, nxk))
        dS, dR, dD = blk("S", k, (nuk, nxk)), blk("R", k, (nuk, nuk)), blk("D", k, (ngk, nuk))
        tq = [sym(dQ) @ x, dS.T @ u, dC.T @ w]
        cd = [-(dC @ x), -(dD @ u)]
        if k < N:
            nx1 = nx[k + 1]
            pi = np.asarray(z["pi"][k])[:nx1]
            dA, dB = blk("A", k, (nx1, nxk)), blk("B", k, (nx1, nuk))
            put("b", k, [dA @ x, dB @ u])
            put("r", k, [sym(dR) @ u, dS @ x, dB.T @ pi, dD.T @ w])
            tq.append(dA.T @ pi)
        put("q", k, tq)
        put("lb", k, [np.zeros(nb[k])])
        put("ub", k, [np.zeros(nb[k])])
        put("lg", k, list(cd))
        put("ug", k, list(cd))
    cat = lambda v: np.concatenate([np.asarray(a, dtype=np.float64).ravel() for a in v] + [np.zeros(0)])
    return {key: cat(out[key]) for key in VEC_KEYS}, mag


class DirRefs:
    """Reference seeds and tangents of the matrix directions, computed once per key and shared (never modified)."""

    def __init__(self, oracle):
        self.mat = MC.shared(oracle)
        self.adj = self.mat.adj
        self.tan = self.adj.tan
        self.apis = self.tan.apis
        self.cache = {}

    def ipm(self, case, seed):
        return self.tan.ipm(case, seed)

    def dtheta(self, case, seed):
        """the problem's matrix direction {key: per-stage blocks}, dQ and dR not symmetric"""
        key = ("dth", case, seed)
        if key not in self.cache:
            P = self.ipm(case, seed)[0]
            rng = np.random.default_rng(11 + seed)
            self.cache[key] = {m: [SCALE * rng.standard_normal(np.shape(M)) for M in P[m]] for m in MAT_KEYS}
        return self.cache[key]

    def seed(self, case, seed, keys=MAT_KEYS):
        """(dF of liboracle.so, of liboracle_fma.so): the oracle's residual difference for the blocks of `keys` moved
        by dtheta_sym, as dense vectors {b, q, r, lb, ub, lg, ug}"""
        ck = ("dF", case, seed, tuple(keys))
        if ck not in self.cache:
            P, *ipms = self.ipm(case, seed)
            P2 = moved_all(P, sym_part(self.dtheta(case, seed)), keys)
            out = []
            for api, z, base in zip(self.apis, ipms, self.mat.base_residuals(case, seed)):
                r = MC.residuals_at(api, P2, z)
                out.append({c: r[c] - base[c] for c in VEC_KEYS})
            self.cache[ck] = tuple(out)
        return self.cache[ck]

    def delta(self, case, seed, build=0):
        """the full reference direction in the vectors: dF of that build plus kkt_tangent_cases' vector delta"""
        P = self.ipm(case, seed)[0]
        return add_delta(P, self.seed(case, seed)[build], self.tan.delta(case, seed))

    def tangent(self, case, seed):
        """(reference tangent of liboracle.so, of liboracle_fma.so), each for its own build's dF: dense dicts"""
        return tuple(self.tan.tangent_of(case, seed, self.delta(case, seed, b), ("matdir", b))[b]
                     for b in range(len(self.apis)))

    def gate(self, ref, alt):
        """the GATES rule from the two builds' spread on one problem"""
        return max(TOL_IPM, 4 * TC.dense_err(alt, ref))

    def measure(self, case):
        """Per usable seed: the two builds' spread on the reference tangent, max |dlam_ref|, and the size of the C and
        of the D direction's residual move."""
        rows = []
        for seed in self.tan.usable(case):
            ref, alt = self.tangent(case, seed)
            big = lambda dF: float(max(np.max(np.abs(dF[c]), initial=0.0) for c in VEC_KEYS))
            rows.append(dict(seed=seed, spread=TC.dense_err(alt, ref),
                             dlam=float(np.max(np.abs(ref["lam"]), initial=0.0)),
                             dFC=big(self.seed(case, seed, ("C",))[0]), dFD=big(self.seed(case, seed, ("D",))[0])))
        return rows

    def usable(self, case):
        """The seeds of the case a test may use, with the three preconditions asserted."""
        key = ("usable", case)
        if key not in self.cache:
            seeds = self.tan.usable(case)
            rows = self.measure(case)
            assert [r["seed"] for r in rows] == seeds and len(seeds) >= len(TC.SEEDS) - 1, (case, seeds)
            for r in rows:
                assert r["spread"] <= TOL_IPM / 4, (case, r)
                if case in GENERAL:
                    assert r["dFC"] > 0.0 and r["dFD"] > 0.0, (case, r)
            if case in GENERAL:
                assert sum(r["dlam"] >= DLAM_ACTIVE for r in rows) >= MIN_ACTIVE, (case, rows)
            self.cache[key] = seeds
        return self.cache[key]


_SHARED = {}


def shared(oracle):
    """One DirRefs per oracle for the whole test session: the host and the GPU module compute the references once."""
    if id(oracle) not in _SHARED:
        _SHARED[id(oracle)] = (oracle, DirRefs(oracle))
    return _SHARED[id(oracle)][1]

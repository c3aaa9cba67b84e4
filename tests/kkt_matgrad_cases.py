"""Shared by tests/test_kkt_matgrad_host.py (CPU) and tests/test_gpu_kkt_matgrad.py: the reference gradients with
respect to the dense matrices A, B, Q, S, R, C, D and the preconditions every test on them asserts.  Oracle only;
nothing here loads the HIP library.

Problems, IPM settings, cotangents and the reference tangent matrix T_ref are kkt_adjoint_cases' (AdjRefs).  The
reference gradient of matrix element (key, k, i, j) is g' T_ref dF: dF is the difference of the oracle's residuals
(d_res_res_mpc_hard_tv, at the oracle IPM's final iterate) between the problem with that element moved by one and the
problem itself, laid out in T_ref's column order -- r_b on b, r_q on [r | q], r_d on [lb | ub | lg | ug], each with the
unit coefficient the residuals give b, q and d.  For Q and R the perturbation is the symmetric pair E_ij + E_ji, halved
off the diagonal.  No outer-product formula enters: the residuals are evaluated by the oracle, element by element.

Preconditions (`usable`):
  1. the problems used are exactly AdjRefs.usable(case) (which asserts its own three): at most 1 of 10 left out;
  2. the reference gradients of the two oracle builds differ by at most TOL_IPM / 4 on every used problem;
  3. on every case with general constraints (ocp_batch_cases.GENERAL: V and E) every used problem has max |gC_ref| >=
     1e-2 and max |gD_ref| >= 1e-2 (the constraint blocks are exercised).
Gate of a comparison against the reference (the GATES rule): max(TOL_IPM, 4 x the two builds' spread on that
problem), relative to max(1, |ref|).  No gate comes from the product's output.

Cost.  The reference moves one matrix element at a time through the oracle's residual routine: 912 to 2416 elements
per problem of the wide cases H, E, B, about 2 s per problem (1 to 3.5 s measured).  For those three cases (WIDE) the
reference gradients are computed for the first N_WIDE = 3 seeds of AdjRefs.usable(case) and those three problems are
compared -- the vector gradients that test_adjoint_data_matches_the_reference checks beside them too, which
test_adjoint_matches_the_reference compares on all ten.  AdjRefs.usable itself still runs over all ten seeds, and
that is where the 1-of-10 cap is asserted.  V, V0, F and S stay at ten.  Measured on those three seeds: worst build
spread H 3.1e-13, E 6.5e-12, B 9.5e-15; on E max |gC_ref| >= 1.35 and max |gD_ref| >= 0.45.
"""
import numpy as np

import kkt_adjoint_cases as AC
from helpers import TOL_IPM
from hpmpc_amd.cabi import bq_from_qp
from hpmpc_amd.ocp_batch import MAT_KEYS, VEC_KEYS, flatten_problems
from ocp_batch_cases import GENERAL, IO

CASES = AC.CASES
WIDE, N_WIDE = ("H", "E", "B"), 3  # the cases whose reference gradients are computed for the first three seeds only
CD_ACTIVE = 1e-2
SYM_KEYS = ("Q", "R")


def residual_columns(P, res):
    """The oracle's residuals of one problem in T_ref's column order: {key: vector} over b, q, r, lb, ub, lg, ug."""
    N, nx, nu, nb, ng = P["N"], P["nx"], P["nu"], P["nb"], P["ng"]
    cat = lambda v: np.concatenate([np.asarray(x, dtype=np.float64).ravel() for x in v] + [np.zeros(0)])
    pnb = [(n + 3) // 4 * 4 for n in nb]
    png = [(n + 3) // 4 * 4 for n in ng]
    K = range(N + 1)
    rq, rb, rd = res["rq"], res["rb"], res["rd"]
    return dict(b=cat([rb[k][:nx[k + 1]] for k in range(N)]), r=cat([rq[k][:nu[k]] for k in range(N)]),
                q=cat([rq[k][nu[k]:nu[k] + nx[k]] for k in K]), lb=cat([rd[k][:nb[k]] for k in K]),
                ub=cat([rd[k][pnb[k]:pnb[k] + nb[k]] for k in K]),
                lg=cat([rd[k][2 * pnb[k]:2 * pnb[k] + ng[k]] for k in K]),
                ug=cat([rd[k][2 * pnb[k] + png[k]:2 * pnb[k] + png[k] + ng[k]] for k in K]))


def residuals_at(api, P, z):
    """residual_columns of problem P at the iterate z (the oracle's padded ux, pi, lam, t lists)"""
    qp = IO.to_qp(P)
    b, q = bq_from_qp(qp)
    return residual_columns(P, api.residuals(qp, b, q, z["ux"], z["pi"], z["lam"], z["t"]))


def moved(P, key, k, M):
    """P with stage k's block of matrix `key` moved by M (every other block shared)."""
    Q = dict(P)
    Q[key] = list(P[key])
    Q[key][k] = np.asarray(P[key][k], dtype=np.float64) + M
    return Q


def unit(shape, i, j, sym):
    """The perturbation of element (i, j): E_ij, or for a symmetric block the pair E_ij + E_ji, halved off the
    diagonal"""
    E = np.zeros(shape)
    if sym and i != j:
        E[i, j] = E[j, i] = 0.5
    else:
        E[i, j] = 1.0
    return E


def dot(a, b, keys):
    return float(sum(np.sum(np.asarray(a[key]) * np.asarray(b[key])) for key in keys))


def mat_err(got, ref):
    """max over A, B, Q, S, R, C, D of |got - ref| / max(1, |ref|); got / ref: {key: per-stage blocks}"""
    return max(AC.rel(np.asarray(g), np.asarray(r)) for key in MAT_KEYS for g, r in zip(got[key], ref[key]))


def flat(P, G, order):
    """Per-stage gradient blocks of one problem -> {key: vector} in the dense layout of OcpBatchSolver"""
    full = dict({s: P[s] for s in AC.SIZE_KEYS}, **{key: G[key] for key in MAT_KEYS})
    return {key: v[0] for key, v in flatten_problems([full], order, keys=MAT_KEYS).items()}


def formulas(P, z, adj):
    """The seven outer products of include/hpmpc_mi355x.h in numpy: z the base iterate (padded ux, pi, lam per stage),
    adj the dense adjoint solution {b, q, r, lb, ub, lg, ug} of one cotangent -> {key: per-stage blocks}."""
    N, nx, nu, nb, ng = P["N"], P["nx"], P["nu"], P["nb"], P["ng"]
    a = AC.per_stage(P, adj, keys=VEC_KEYS)
    G = {key: [] for key in MAT_KEYS}
    for k in range(N + 1):
        nuk = nu[k] if k < N else 0
        pnb, png = (nb[k] + 3) // 4 * 4, (ng[k] + 3) // 4 * 4
        u, x = np.asarray(z["ux"][k])[:nuk], np.asarray(z["ux"][k])[nuk:nuk + nx[k]]
        rbar, qxbar = (a["r"][k] if k < N else np.zeros(0)), a["q"][k]
        lam = np.asarray(z["lam"][k])
        w = lam[2 * pnb + png:2 * pnb + png + ng[k]] - lam[2 * pnb:2 * pnb + ng[k]]
        s = a["lg"][k] + a["ug"][k]
        if k < N:
            bbar, pi = a["b"][k], np.asarray(z["pi"][k])[:nx[k + 1]]
            G["A"].append(np.outer(bbar, x) + np.outer(pi, qxbar))
            G["B"].append(np.outer(bbar, u) + np.outer(pi, rbar))
        G["Q"].append(0.5 * (np.outer(qxbar, x) + np.outer(x, qxbar)))
        G["R"].append(0.5 * (np.outer(rbar, u) + np.outer(u, rbar)))
        G["S"].append(np.outer(rbar, x) + np.outer(u, qxbar))
        G["C"].append(np.outer(w, qxbar) - np.outer(s, x))
        G["D"].append(np.outer(w, rbar) - np.outer(s, u))
    return G


class MatRefs:
    """Reference matrix gradients, computed once per key and shared (never modified)."""

    def __init__(self, oracle):
        self.adj = AC.AdjRefs(oracle)
        self.apis = self.adj.tan.apis
        self.cache = {}

    def ipm(self, case, seed):
        return self.adj.ipm(case, seed)

    def base_residuals(self, case, seed):
        """residual_columns of the problem at each build's own final IPM iterate"""
        key = ("res", case, seed)
        if key not in self.cache:
            P, *ipms = self.ipm(case, seed)
            self.cache[key] = tuple(residuals_at(api, P, z) for api, z in zip(self.apis, ipms))
        return self.cache[key]

    def residual_delta(self, case, seed, key, k, M):
        """(dF of liboracle.so, of liboracle_fma.so) for stage k's block of `key` moved by M"""
        P, *ipms = self.ipm(case, seed)
        P2 = moved(P, key, k, M)
        out = []
        for api, z, base in zip(self.apis, ipms, self.base_residuals(case, seed)):
            r = residuals_at(api, P2, z)
            out.append({c: r[c] - base[c] for c in VEC_KEYS})
        return tuple(out)

    def gradients(self, case, seed):
        """(reference of liboracle.so, of liboracle_fma.so): {key: per-stage blocks} for the problem's own cotangent"""
        ck = ("G", case, seed)
        if ck not in self.cache:
            P = self.ipm(case, seed)[0]
            adj = self.adj.adjoint(case, seed)  # T_ref' g of each build
            out = tuple({key: [np.zeros(np.shape(M)) for M in P[key]] for key in MAT_KEYS} for _ in self.apis)
            for key in MAT_KEYS:
                sym = key in SYM_KEYS
                for k, M in enumerate(P[key]):
                    m, n = np.shape(M)
                    for i in range(m):
                        for j in range(i + 1 if sym else n):  # a symmetric pair is one perturbation
                            dF = self.residual_delta(case, seed, key, k, unit((m, n), i, j, sym))
                            for b in range(len(self.apis)):
                                out[b][key][k][i, j] = dot(adj[b], dF[b], VEC_KEYS)
                                if sym:
                                    out[b][key][k][j, i] = out[b][key][k][i, j]
            self.cache[ck] = out
        return self.cache[ck]

    def gate(self, ref, alt):
        """the GATES rule from the two builds' spread on one problem"""
        return max(TOL_IPM, 4 * mat_err(alt, ref))

    def seeds(self, case):
        """AdjRefs.usable(case) (asserted there over all ten seeds); of a WIDE case its first N_WIDE"""
        seeds = self.adj.usable(case)
        return seeds[:N_WIDE] if case in WIDE else seeds

    def measure(self, case):
        """Per usable seed: the two builds' spread on the reference gradients, their element count, max |gC|, |gD|."""
        rows = []
        for seed in self.seeds(case):
            ref, alt = self.gradients(case, seed)
            big = lambda key: float(max([np.max(np.abs(M), initial=0.0) for M in ref[key]] + [0.0]))
            rows.append(dict(seed=seed, spread=mat_err(alt, ref), nel=sum(M.size for key in MAT_KEYS for M in ref[key]),
                             gC=big("C"), gD=big("D")))
        return rows

    def usable(self, case):
        """The seeds of the case a test may use, with the three preconditions asserted."""
        key = ("usable", case)
        if key not in self.cache:
            full = self.adj.usable(case)
            assert len(full) >= len(AC.TC.SEEDS) - 1, (case, full)
            seeds = self.seeds(case)
            rows = self.measure(case)
            assert [r["seed"] for r in rows] == seeds, (case, seeds)
            for r in rows:
                assert r["spread"] <= TOL_IPM / 4, (case, r)
                if case in GENERAL:
                    assert r["gC"] >= CD_ACTIVE and r["gD"] >= CD_ACTIVE, (case, r)
            self.cache[key] = seeds
        return self.cache[key]


_SHARED = {}


def shared(oracle):
    """One MatRefs per oracle for the whole test session: the host and the GPU module compute the references once."""
    if id(oracle) not in _SHARED:
        _SHARED[id(oracle)] = (oracle, MatRefs(oracle))
    return _SHARED[id(oracle)][1]

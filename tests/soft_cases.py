"""Shared by tests/test_soft_cases_host.py, tests/test_gpu_soft.py, tests/test_gpu_soft_batch.py and
tests/golden/make_golden.py: the soft-constraint IPM on random stage structure (hpmpc_amd.soft.random_soft_qp), the
admitted (case, seed) pairs with the oracle's iteration counts, and a restatement of where the reference's stray
soft-gradient write lands (hpmpc_capi_soft.cpp soft_layout).

Admission rule (a condition on the CPU builds; tests/test_soft_cases_host.py checks it on the two oracle builds, and
make_golden.py soft_admission prints it with the reference's c99 build beside them): a (case, seed) pair is used only
if the reference build, the oracle and the oracle's FMA build return identical kk and ret, the two oracle builds
differ by at most 25 % of every TOL_SOFT gate, and the run either converges (ret 0) or is the early exit of `x0_box`
(ret 2 at kk <= 4: a variable x_0 with boxes on its states).  Every draw below uses structure_seed 0 and the case's
own x0_scale.  No test takes a divergence escape.
"""
import numpy as np

from helpers import TOL_SOFT
from hpmpc_amd.soft import random_soft_qp

ARGS = dict(k_max=50, mu0=100.0, mu_tol=1e-6, alpha_min=1e-8)
ADMIT = 0.25  # oracle build spread, as a share of each TOL_SOFT gate

# name -> sizes (N, nx, nu, nb, ns), generator options, and the admitted draws as (seed, kk, ret, spread): kk / ret
# are the oracle's (identical in its FMA build and in the reference's c99 build), spread the worst distance of the two
# oracle builds as a share of its TOL_SOFT gate, measured when the seed was admitted (make_golden.py soft_admission).
CASES = {
    # odd nx, varying stages, two four-stage sweeps, stray writes into stage 6's live qx
    "odd": dict(N=6, nx=[0, 3, 7, 4, 8, 11, 3], nu=[2, 3, 1, 4, 2, 4, 0], nb=[1, 2, 0, 3, 2, 4, 1],
                ns=[0, 3, 5, 2, 7, 6, 2], kw={},
                draws=[(1, 7, 0, 1.1e-8), (2, 6, 0, 6.3e-8), (3, 8, 0, 7.5e-3), (6, 7, 0, 2.1e-3), (7, 8, 0, 3.6e-3)]),
    # soft boxes on inputs; inner stages with nb = 0, ns > 0
    "soft_u": dict(N=5, nx=[0, 4, 4, 8, 8, 4], nu=[3, 3, 2, 4, 4, 0], nb=[0, 2, 3, 1, 0, 0],
                   ns=[2, 4, 3, 6, 9, 3], kw={},
                draws=[(2, 7, 0, 4.1e-6), (3, 7, 0, 1.1e-6), (5, 8, 0, 6.9e-2)]),
    # variable x_0
    "x0_u": dict(N=4, nx=[4] * 5, nu=[2, 2, 2, 2, 0], nb=[2, 2, 2, 2, 0], ns=[0, 4, 4, 4, 4],
                 kw=dict(x0_scale=0.05),
                draws=[(0, 6, 0, 5.2e-8), (1, 5, 0, 4.4e-8), (2, 5, 0, 2.3e-8)]),
    # variable x_0 with boxes on its states: the early ret-2 exit
    "x0_box": dict(N=4, nx=[4, 4, 7, 7, 8], nu=[2, 2, 3, 1, 0], nb=[3, 2, 0, 4, 3], ns=[3, 4, 7, 3, 5],
                   kw=dict(x0_scale=0.05),
                draws=[(0, 3, 2, 4.0e-8), (1, 2, 2, 1.0e-7), (2, 3, 2, 3.8e-8), (3, 3, 2, 1.1e-8)]),
    # all 16 slots, in three hard / soft splits
    "full16": dict(N=4, nx=[0, 12, 12, 12, 8], nu=[4, 4, 4, 4, 0], nb=[4, 7, 3, 0, 0], ns=[0, 9, 13, 16, 8],
                   kw=dict(x0_scale=0.3),
                draws=[(0, 6, 0, 2.2e-8), (1, 5, 0, 3.0e-8), (2, 6, 0, 6.7e-9)]),
    # no hard box anywhere
    "softonly": dict(N=3, nx=[0, 4, 3, 4], nu=[1, 2, 1, 0], nb=[0] * 4, ns=[1, 5, 2, 3], kw={},
                draws=[(0, 7, 0, 4.9e-3), (1, 7, 0, 6.7e-3), (6, 7, 0, 1.4e-2), (7, 6, 0, 6.4e-5)]),
    # shortest horizon
    "N1": dict(N=1, nx=[0, 3], nu=[2, 0], nb=[1, 2], ns=[1, 1], kw={},
                draws=[(1, 7, 0, 2.5e-2), (2, 8, 0, 4.3e-6), (3, 9, 0, 2.1e-3), (7, 6, 0, 4.5e-4)]),
    # stray writes of stage 1 into qx of stage 2 (same sweep, nb = 0 there), of stage 5 into qx of stage 6
    "stray": dict(N=6, nx=[0, 7, 7, 4, 4, 8, 4], nu=[2, 3, 1, 4, 2, 2, 0], nb=[2, 3, 0, 3, 0, 2, 1],
                  ns=[0, 6, 2, 5, 2, 7, 2], kw={},
                draws=[(1, 8, 0, 6.0e-3), (2, 9, 0, 1.8e-2), (3, 8, 0, 8.5e-2)]),
}


def make(case, seed, **over):
    c = CASES[case]
    kw = dict(c["kw"])
    kw.update(over)
    return random_soft_qp(c["N"], c["nx"], c["nu"], c["nb"], c["ns"], seed=seed, **kw)


def seeds(case):
    return [d[0] for d in CASES[case]["draws"]]


def kks(case):
    return [d[1] for d in CASES[case]["draws"]]


def problems(case):
    """The admitted draws of a case: one batch (they share sizes and idxb)."""
    return [make(case, s) for s in seeds(case)]


def refusal_shape():
    """N = 2, boxes and soft boxes on stage N only (nb = ns = 4, nx = 8): the reference's soft-gradient write of
    stage N lands at Zl_N[4..7], which its own loop reads right after."""
    return random_soft_qp(2, [0, 8, 8], [2, 2, 0], [0, 0, 4], [0, 0, 4], seed=0)


WARM_KK = 7  # `odd` at its first admitted seed, warm-started from warm_ux: kk of the three builds (spread 2.0e-8)


def warm_ux(sq, seed=4):
    rng = np.random.default_rng(seed)
    return [0.05 * rng.standard_normal(sq.nux(k) + 4) for k in range(sq.N + 1)]


def soft_errors(sq, a, b):
    """Worst |a - b| / max(1, |b|) of two ipm_soft results per gated vector (the valid entries), or None when kk / ret
    differ: the distances tests/test_gpu_soft.py _cmp asserts."""
    if a["ret"] != b["ret"] or a["kk"] != b["kk"]:
        return None
    rel = lambda g, r: float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r)), initial=0.0))
    e = dict(ux=0.0, pi=0.0, lam=0.0, t=0.0, stat=rel(np.asarray(a["stat"]), np.asarray(b["stat"])))
    for k in range(sq.N + 1):
        n = sq.nux(k)
        e["ux"] = max(e["ux"], rel(a["ux"][k][:n], b["ux"][k][:n]))
        if k < sq.N:
            m = int(sq.nx[k + 1])
            e["pi"] = max(e["pi"], rel(a["pi"][k][:m], b["pi"][k][:m]))
        nb, ns = int(sq.nb[k]), int(sq.ns[k])
        pnb, pns = (nb + 3) // 4 * 4, (ns + 3) // 4 * 4
        idx = np.concatenate([np.arange(nb), np.arange(pnb, pnb + nb)] +
                             [np.arange(2 * pnb + s * pns, 2 * pnb + s * pns + ns) for s in range(4)]).astype(int)
        for key in ("lam", "t"):
            e[key] = max(e[key], rel(np.asarray(a[key][k])[idx], np.asarray(b[key][k])[idx]))
    return e


def gate_share(e):
    """The errors of soft_errors as shares of their TOL_SOFT gates; inf where kk / ret differ."""
    return {k: float("inf") for k in TOL_SOFT} if e is None else {k: e[k] / TOL_SOFT[k] for k in TOL_SOFT}


def soft_stray_targets(sq):
    """Where the reference's soft corrector gradient lands (d_aux_ip_soft_lib4.c:557, :601), restated from the flat
    carve of d_ip2_soft.c:244-260 as hpmpc_capi_soft.cpp soft_layout holds it: Qx_k | qx_k (pnb + pns doubles each)
    for k = 0..N, then Zl_k | zl_k (2 pns each) for k = 0..N.  With nb > 0 the term of soft box i of stage k is added
    at qx_k + round_up(nb + ns, 4) + nb + i, past the slot the Riccati reads (with nb = 0 it goes to its own slot i
    and is no stray).  Returns (targets, refused): one dict per stray element with its source stage k and element i,
    the array ("Qx", "qx", "Zl", "zl", or "pad" beyond the carve) and stage j it lands in, the offset there, and
    `live`: whether that slot belongs to a real box or soft box; refused restates soft_layout's refusal (a write into
    the Zl half of a stage j >= k, which the same pass reads later)."""
    N = sq.N
    r4 = lambda n: (int(n) + 3) // 4 * 4
    nb, ns = [int(v) for v in sq.nb], [int(v) for v in sq.ns]
    pnb, pns = [r4(v) for v in nb], [r4(v) for v in ns]
    oQ, oZl, F = [], [], 0
    for k in range(N + 1):
        oQ.append(F)
        F += 2 * (pnb[k] + pns[k])
    for k in range(N + 1):
        oZl.append(F)
        F += 4 * pns[k]
    out, refused = [], False
    for k in range(N + 1):
        if nb[k] == 0:
            continue
        oS = oQ[k] + pnb[k] + pns[k] + r4(nb[k] + ns[k]) + nb[k]
        for i in range(ns[k]):
            pos = oS + i
            hit = dict(k=k, i=i, pos=pos, array="pad", j=None, off=None, live=False)
            for j in range(N + 1):
                w = pnb[j] + pns[j]
                if oQ[j] <= pos < oQ[j] + 2 * w:
                    off = pos - oQ[j]
                    hit.update(array="Qx" if off < w else "qx", j=j, off=off % w, live=off % w < nb[j] + ns[j])
                elif oZl[j] <= pos < oZl[j] + 4 * pns[j]:
                    off = pos - oZl[j]
                    hit.update(array="Zl" if off < 2 * pns[j] else "zl", j=j, off=off % (2 * pns[j]),
                               live=off % pns[j] < ns[j])
            if hit["array"] == "Zl" and hit["j"] >= k:
                refused = True
            out.append(hit)
    return out, refused

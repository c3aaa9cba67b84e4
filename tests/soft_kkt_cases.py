"""Shared by tests/test_soft_kkt_host.py and tests/test_gpu_soft_kkt.py: the batched soft KKT re-solve
(hpmpc_mi355x_soft_kkt_batch / hpmpc_mi355x_soft_kkt_ocp_batch, include/hpmpc_mi355x.h) against a numpy reference.

A linearisation is (Lam, tau) in the layout of lam, per stage [lo pnb | up pnb | s0 s1 s2 s3 (pns each)].  For one set
(b, q, r, lb, ub, z in interface form) ``newton_reference`` assembles the un-eliminated Newton system in (w, pi, s, t',
lam') -- stationarity, dynamics, the constraint rows, lam' = Lam (tau - t') and the slack stationarity rows -- and solves
it with np.linalg.solve; ``newton_eliminated`` eliminates slacks and multipliers first (Qx, qx, Zl, zl as the soft IPM's
Hessian update forms them, with lam = Lam tau) and solves the KKT system in (w, pi) alone.

Cases are interface-form problems through tests/ocp_soft_cases.make.  A draw is a seed 0 .. 9: the problem of that seed,
a base (lam, t) from U[0.5, 2] on the live slots (padding: t = 1, lam = 0, so Lam is in [0.25, 4]) and NSETS sets, seeded
perturbations of the problem's own vectors (b, q, r +- 0.1 N(0,1); bounds widened by 0.1 |N(0,1)|; z + 0.1 |N(0,1)|).

Admission rule (tests/test_soft_kkt_host.py checks it; in the spirit of soft_cases.ADMIT): a draw is used only if on
every set the two formulations agree within 25 % of each TOL_SOFT gate and the residuals of the reference solution on the
set's own data vanish: max |r_q|, |r_b|, |r_d|, |r_z| <= 1e-9 max(1, largest |entry| of the set's vectors).  A draw that
fails is skipped in favour of the next seed; a case keeps the first MAX_DRAWS admitted draws and needs MIN_DRAWS.
"""
import numpy as np

import ocp_soft_cases as OC
from helpers import TOL_SOFT
from hpmpc_amd.ocp import rup
from hpmpc_amd.soft import soft_batch_layout

CASES = ("D", "Q", "N1", "softonly", "odd", "full16", "x0_u", "stray", "iface_soft_N12_nx8_nu3")
# the shapes where idxb[k][nu + i] and idxb[k][nb + i] coincide (nb = nu on every stage with soft boxes): the oracle's
# d_res_mpc_soft_tv reads the soft variable where the IPM puts it
ORACLE_RES = ("D", "iface_soft_N12_nx8_nu3")
SEEDS = range(10)
NSETS = 3
MIN_DRAWS, MAX_DRAWS = 3, 6
ADMIT = 0.25
RES_TOL = 1e-9
SET_KEYS = ("b", "q", "r", "lb", "ub", "z")
# admitted draws per case, recorded when the rule was last evaluated (tests/test_soft_kkt_host.py asserts them)
ADMITTED = {c: [0, 1, 2, 3, 4, 5] for c in CASES}


def sizes(P, k):
    nu, nx, nb, ns = P["nu"][k] if k < P["N"] else 0, P["nx"][k], P["nb"][k], P["ns"][k]
    return nu, nx, nb, ns, rup(nb, 4), rup(ns, 4)


def live_slots(P, k):
    """Indices of the live entries of stage k's lam / t: [lo nb | up nb | 4 x ns] inside [lo pnb | up pnb | 4 x pns]."""
    _, _, nb, ns, pnb, pns = sizes(P, k)
    return np.concatenate([np.arange(nb), pnb + np.arange(nb)] +
                          [2 * pnb + j * pns + np.arange(ns) for j in range(4)]).astype(int)


def draw(case, seed, nsets=NSETS):
    """(P, lam, t, sets): the problem of ``seed``, the base iterate (per-stage padded lists) and ``nsets`` sets."""
    P = OC.make(case, seed)
    rng = np.random.Generator(np.random.PCG64(1000 + seed))
    N = P["N"]
    lam, t = [], []
    for k in range(N + 1):
        _, _, nb, ns, pnb, pns = sizes(P, k)
        lk, tk = np.zeros(2 * pnb + 4 * pns), np.ones(2 * pnb + 4 * pns)
        idx = live_slots(P, k)
        lk[idx] = rng.uniform(0.5, 2.0, idx.size)
        tk[idx] = rng.uniform(0.5, 2.0, idx.size)
        lam.append(lk)
        t.append(tk)
    sets = []
    for _ in range(nsets):
        S = {}
        for key in ("b", "q", "r"):
            S[key] = [np.asarray(v, dtype=np.float64) + 0.1 * rng.standard_normal(np.shape(v)) for v in P[key]]
        S["lb"] = [np.asarray(v, dtype=np.float64) - 0.1 * np.abs(rng.standard_normal(np.shape(v))) for v in P["lb"]]
        S["ub"] = [np.asarray(v, dtype=np.float64) + 0.1 * np.abs(rng.standard_normal(np.shape(v))) for v in P["ub"]]
        S["z"] = [np.asarray(v, dtype=np.float64) + 0.1 * np.abs(rng.standard_normal(np.shape(v))) for v in P["z"]]
        sets.append(S)
    return P, lam, t, sets


def with_set(P, S):
    """The interface-form problem ``P`` with the vectors of set ``S`` in place of its own."""
    Q = dict(P)
    for key in SET_KEYS:
        Q[key] = S[key]
    return Q


def set_scale(S):
    return max(1.0, max((float(np.max(np.abs(v), initial=0.0)) for key in SET_KEYS for v in S[key]), default=0.0))


def _stage_mats(P, k):
    """H_k over [u | x], g's matrix part, and BAbt_k = [B' ; A'] (nux x nx1; None at k = N)."""
    N = P["N"]
    nu, nx = (P["nu"][k] if k < N else 0), P["nx"][k]
    H = np.zeros((nu + nx, nu + nx))
    H[nu:, nu:] = np.asarray(P["Q"][k]).reshape(nx, nx)
    if k < N and nu:
        H[:nu, :nu] = np.asarray(P["R"][k]).reshape(nu, nu)
        Sk = np.asarray(P["S"][k]).reshape(nu, nx)
        H[:nu, nu:] = Sk
        H[nu:, :nu] = Sk.T
    Bt = None
    if k < N:
        nx1 = P["nx"][k + 1]
        Bt = np.vstack([np.asarray(P["B"][k]).reshape(nx1, nu).T, np.asarray(P["A"][k]).reshape(nx1, nx).T])
    return H, Bt


def _grad(P, S, k):
    nu = P["nu"][k] if k < P["N"] else 0
    return np.r_[np.asarray(S["r"][k])[:nu] if k < P["N"] else np.zeros(0), np.asarray(S["q"][k])]


def newton_reference(P, Lam, tau, S):
    """The un-eliminated system.  Returns dict ux, pi (per-stage lists), lam, t (per-stage padded lists), s (per-stage
    [lower ns | upper ns])."""
    N = P["N"]
    ow, op, oc, n = [], [], [], 0
    for k in range(N + 1):
        nu, nx, nb, ns, _, _ = sizes(P, k)
        ow.append(n)
        n += nu + nx
    for k in range(N):
        op.append(n)
        n += P["nx"][k + 1]
    for k in range(N + 1):  # per hard box: t_lo t_up l_lo l_up; per soft box: s_l s_u t0..3 l0..3
        _, _, nb, ns, _, _ = sizes(P, k)
        oc.append(n)
        n += 4 * nb + 10 * ns
    M, rhs = np.zeros((n, n)), np.zeros(n)
    row = 0
    for k in range(N + 1):
        nu, nx, nb, ns, pnb, pns = sizes(P, k)
        nux, ib = nu + nx, np.asarray(P["hidxb"][k])
        H, Bt = _stage_mats(P, k)
        # stationarity: H w + g - [0; pi_{k-1}] + BAbt pi_k - sum e_v (l_lo - l_up) - sum e_v (l_0 - l_1) = 0
        r0 = row
        M[r0:r0 + nux, ow[k]:ow[k] + nux] = H
        rhs[r0:r0 + nux] = -_grad(P, S, k)
        if k > 0:
            M[r0 + nu:r0 + nux, op[k - 1]:op[k - 1] + nx] -= np.eye(nx)
        if k < N:
            M[r0:r0 + nux, op[k]:op[k] + P["nx"][k + 1]] += Bt
        for j in range(nb):
            c = oc[k] + 4 * j
            M[r0 + ib[j], c + 2] -= 1.0
            M[r0 + ib[j], c + 3] += 1.0
        for i in range(ns):
            c = oc[k] + 4 * nb + 10 * i
            M[r0 + ib[nb + i], c + 6] -= 1.0
            M[r0 + ib[nb + i], c + 7] += 1.0
        row += nux
        if k < N:  # dynamics: x_{k+1} - BAbt' w_k = b
            nx1, nu1 = P["nx"][k + 1], (P["nu"][k + 1] if k + 1 < N else 0)
            M[row:row + nx1, ow[k + 1] + nu1:ow[k + 1] + nu1 + nx1] = np.eye(nx1)
            M[row:row + nx1, ow[k]:ow[k] + nux] -= Bt.T
            rhs[row:row + nx1] = np.asarray(S["b"][k])
            row += nx1
        lb, ub, L, T = np.asarray(S["lb"][k]), np.asarray(S["ub"][k]), Lam[k], tau[k]
        for j in range(nb):
            c, v = oc[k] + 4 * j, ow[k] + ib[j]
            M[row, c], M[row, v], rhs[row] = 1.0, -1.0, -lb[j]  # t_lo = w - lb
            M[row + 1, c + 1], M[row + 1, v], rhs[row + 1] = 1.0, 1.0, ub[j]  # t_up = ub - w
            for h, e in ((0, j), (1, pnb + j)):  # l + Lam t = Lam tau
                M[row + 2 + h, c + 2 + h], M[row + 2 + h, c + h], rhs[row + 2 + h] = 1.0, L[e], L[e] * T[e]
            row += 4
        Z, z = np.asarray(P["Z"][k]), np.asarray(S["z"][k])
        for i in range(ns):
            c, v = oc[k] + 4 * nb + 10 * i, ow[k] + ib[nb + i]
            sl, su, t0, l0 = c, c + 1, c + 2, c + 6
            M[row, t0], M[row, v], M[row, sl], rhs[row] = 1.0, -1.0, -1.0, -lb[nb + i]  # t0 = w - ls + s_l
            M[row + 1, t0 + 1], M[row + 1, v], M[row + 1, su], rhs[row + 1] = 1.0, 1.0, -1.0, ub[nb + i]
            M[row + 2, t0 + 2], M[row + 2, sl] = 1.0, -1.0  # t2 = s_l
            M[row + 3, t0 + 3], M[row + 3, su] = 1.0, -1.0
            for h in range(4):
                e = 2 * pnb + h * pns + i
                M[row + 4 + h, l0 + h], M[row + 4 + h, t0 + h], rhs[row + 4 + h] = 1.0, L[e], L[e] * T[e]
            M[row + 8, sl], M[row + 8, l0], M[row + 8, l0 + 2], rhs[row + 8] = Z[i], -1.0, -1.0, -z[i]
            M[row + 9, su], M[row + 9, l0 + 1], M[row + 9, l0 + 3], rhs[row + 9] = Z[ns + i], -1.0, -1.0, -z[ns + i]
            row += 10
    assert row == n
    sol = np.linalg.solve(M, rhs)
    out = dict(ux=[], pi=[], lam=[], t=[], s=[])
    for k in range(N + 1):
        nu, nx, nb, ns, pnb, pns = sizes(P, k)
        out["ux"].append(sol[ow[k]:ow[k] + nu + nx].copy())
        if k < N:
            out["pi"].append(sol[op[k]:op[k] + P["nx"][k + 1]].copy())
        lk, tk, sk = np.zeros(2 * pnb + 4 * pns), np.zeros(2 * pnb + 4 * pns), np.zeros(2 * ns)
        for j in range(nb):
            c = oc[k] + 4 * j
            tk[j], tk[pnb + j], lk[j], lk[pnb + j] = sol[c:c + 4]
        for i in range(ns):
            c = oc[k] + 4 * nb + 10 * i
            sk[i], sk[ns + i] = sol[c], sol[c + 1]
            for h in range(4):
                tk[2 * pnb + h * pns + i], lk[2 * pnb + h * pns + i] = sol[c + 2 + h], sol[c + 6 + h]
        out["lam"].append(lk)
        out["t"].append(tk)
        out["s"].append(sk)
    return out


def newton_eliminated(P, Lam, tau, S):
    """The slack-eliminated formulation: Qx, qx, Zl, zl per box, the KKT system in (w, pi), then t', s, lam'."""
    N = P["N"]
    ow, op, n = [], [], 0
    for k in range(N + 1):
        nu, nx, _, _, _, _ = sizes(P, k)
        ow.append(n)
        n += nu + nx
    for k in range(N):
        op.append(n)
        n += P["nx"][k + 1]
    M, rhs = np.zeros((n, n)), np.zeros(n)
    keep = []
    for k in range(N + 1):
        nu, nx, nb, ns, pnb, pns = sizes(P, k)
        nux, ib = nu + nx, np.asarray(P["hidxb"][k])
        H, Bt = _stage_mats(P, k)
        g = _grad(P, S, k).copy()
        H = H.copy()
        lb, ub, L, T = np.asarray(S["lb"][k]), np.asarray(S["ub"][k]), Lam[k], tau[k]
        Z, z = np.asarray(P["Z"][k]), np.asarray(S["z"][k])
        for j in range(nb):
            ll, lu = L[j], L[pnb + j]
            H[ib[j], ib[j]] += ll + lu
            g[ib[j]] += lu * T[pnb + j] - lu * ub[j] - ll * T[j] - ll * lb[j]
        Zl, zl = np.zeros(2 * ns), np.zeros(2 * ns)
        for i in range(ns):
            lt = [L[2 * pnb + h * pns + i] for h in range(4)]
            la = [lt[h] * T[2 * pnb + h * pns + i] for h in range(4)]
            rq0, rq1 = la[0] + lt[0] * lb[nb + i], la[1] - lt[1] * ub[nb + i]
            Zl[i], Zl[ns + i] = 1.0 / (Z[i] + lt[0] + lt[2]), 1.0 / (Z[ns + i] + lt[1] + lt[3])
            zl[i], zl[ns + i] = -z[i] + rq0 + la[2], -z[ns + i] + rq1 + la[3]
            rq0 -= lt[0] * zl[i] * Zl[i]
            rq1 -= lt[1] * zl[ns + i] * Zl[ns + i]
            v = ib[nb + i]
            H[v, v] += (lt[0] - lt[0] ** 2 * Zl[i]) + (lt[1] - lt[1] ** 2 * Zl[ns + i])
            g[v] += rq1 - rq0
        keep.append((Zl, zl))
        M[ow[k]:ow[k] + nux, ow[k]:ow[k] + nux] = H
        rhs[ow[k]:ow[k] + nux] = -g
        if k > 0:
            M[ow[k] + nu:ow[k] + nux, op[k - 1]:op[k - 1] + nx] -= np.eye(nx)
            M[op[k - 1]:op[k - 1] + nx, ow[k] + nu:ow[k] + nux] -= np.eye(nx)
        if k < N:
            nx1 = P["nx"][k + 1]
            M[ow[k]:ow[k] + nux, op[k]:op[k] + nx1] += Bt
            M[op[k]:op[k] + nx1, ow[k]:ow[k] + nux] += Bt.T
            rhs[op[k]:op[k] + nx1] = -np.asarray(S["b"][k])
    sol = np.linalg.solve(M, rhs)
    out = dict(ux=[], pi=[], lam=[], t=[], s=[])
    for k in range(N + 1):
        nu, nx, nb, ns, pnb, pns = sizes(P, k)
        ib = np.asarray(P["hidxb"][k])
        w = sol[ow[k]:ow[k] + nu + nx].copy()
        out["ux"].append(w)
        if k < N:
            out["pi"].append(sol[op[k]:op[k] + P["nx"][k + 1]].copy())
        lb, ub, L, T = np.asarray(S["lb"][k]), np.asarray(S["ub"][k]), Lam[k], tau[k]
        tk, sk = np.zeros(2 * pnb + 4 * pns), np.zeros(2 * ns)
        for j in range(nb):
            tk[j], tk[pnb + j] = w[ib[j]] - lb[j], ub[j] - w[ib[j]]
        Zl, zl = keep[k]
        for i in range(ns):
            x, o = w[ib[nb + i]], 2 * pnb
            sk[i] = (zl[i] - L[o + i] * x) * Zl[i]
            sk[ns + i] = (zl[ns + i] + L[o + pns + i] * x) * Zl[ns + i]
            tk[o + i], tk[o + pns + i] = sk[i] + x - lb[nb + i], sk[ns + i] - x + ub[nb + i]
            tk[o + 2 * pns + i], tk[o + 3 * pns + i] = sk[i], sk[ns + i]
        lk = np.zeros_like(tk)
        idx = live_slots(P, k)
        lk[idx] = L[idx] * (T[idx] - tk[idx])
        out["lam"].append(lk)
        out["t"].append(tk)
        out["s"].append(sk)
    return out


def rel_errors(P, got, ref):
    """Worst |got - ref| / max(1, |ref|) per gated vector over the live entries."""
    rel = lambda g, r: float(np.max(np.abs(np.asarray(g) - np.asarray(r)) / np.maximum(1.0, np.abs(r)), initial=0.0))
    e = dict(ux=0.0, pi=0.0, lam=0.0, t=0.0)
    for k in range(P["N"] + 1):
        nu, nx, _, _, _, _ = sizes(P, k)
        e["ux"] = max(e["ux"], rel(np.asarray(got["ux"][k])[:nu + nx], ref["ux"][k]))
        if k < P["N"]:
            e["pi"] = max(e["pi"], rel(np.asarray(got["pi"][k])[:P["nx"][k + 1]], ref["pi"][k]))
        idx = live_slots(P, k)
        for key in ("lam", "t"):
            e[key] = max(e[key], rel(np.asarray(got[key][k])[idx], ref[key][k][idx]))
    return e


def gate_share(e):
    return {k: e[k] / TOL_SOFT[k] for k in e}


def residual_max(P, S, sol, reading="nb"):
    """max |r_q|, |r_b|, |r_d|, |r_z| of a solution on the set's own data: d_res_mpc_soft_tv restated in numpy with the
    variable of soft constraint i of stage k read at idxb[k][nb_k + i] (reading "nb": where the IPM puts it) or at
    idxb[k][nu_k + i] ("nu": the reference), and a soft box's multipliers entering r_q as lam_0 - lam_1 on every stage.
    r_d extends ocp_soft_cases.soft_rd_max."""
    N = P["N"]
    PS = with_set(P, S)
    m = dict(rq=0.0, rb=0.0, rz=0.0, rd=OC.soft_rd_max(PS, sol["ux"], sol["t"], reading))
    for k in range(N + 1):
        nu, nx, nb, ns, pnb, pns = sizes(P, k)
        ib = np.asarray(P["hidxb"][k])
        H, Bt = _stage_mats(P, k)
        w, lam, t = np.asarray(sol["ux"][k])[:nu + nx], sol["lam"][k], sol["t"][k]
        rq = H @ w + _grad(P, S, k)
        if k > 0:
            rq[nu:] -= np.asarray(sol["pi"][k - 1])[:nx]
        if k < N:
            pi = np.asarray(sol["pi"][k])[:P["nx"][k + 1]]
            rq += Bt @ pi
            nu1 = P["nu"][k + 1] if k + 1 < N else 0
            x1 = np.asarray(sol["ux"][k + 1])[nu1:nu1 + P["nx"][k + 1]]
            m["rb"] = max(m["rb"], float(np.max(np.abs(x1 - Bt.T @ w - np.asarray(S["b"][k])), initial=0.0)))
        for j in range(nb):
            rq[ib[j]] -= lam[j] - lam[pnb + j]
        o = 2 * pnb
        Z, z = np.asarray(P["Z"][k]), np.asarray(S["z"][k])
        for i in range(ns):
            rq[ib[(nb if reading == "nb" else nu) + i]] -= lam[o + i] - lam[o + pns + i]
            m["rz"] = max(m["rz"], abs(z[i] + Z[i] * t[o + 2 * pns + i] - lam[o + i] - lam[o + 2 * pns + i]),
                          abs(z[ns + i] + Z[ns + i] * t[o + 3 * pns + i] - lam[o + pns + i] - lam[o + 3 * pns + i]))
        m["rq"] = max(m["rq"], float(np.max(np.abs(rq), initial=0.0)))
    return m


def admit(case, seed):
    """(admitted, figures) of one draw: the worst gate share between the two formulations over its sets, and the worst
    residual of the reference solution as a share of RES_TOL * scale."""
    P, lam, t, sets = draw(case, seed)
    Lam = [l / tt for l, tt in zip(lam, t)]
    share, res = 0.0, 0.0
    for S in sets:
        ref, eli = newton_reference(P, Lam, t, S), newton_eliminated(P, Lam, t, S)
        share = max(share, max(gate_share(rel_errors(P, eli, ref)).values()))
        res = max(res, max(residual_max(P, S, ref).values()) / (RES_TOL * set_scale(S)))
    return share <= ADMIT and res <= 1.0, dict(share=share, res=res)


def admitted(case):
    return list(ADMITTED[case])


# ---- the padded arrays of the packed-level call ----

def soft_qps(Ps):
    return [OC.soft_qp(P, True) for P in Ps]


def padded_sets(P, sets):
    """b, q (nrhs, N+1, 16), d (nrhs, sD), z (nrhs, sZ) of one problem's sets in the layouts of the packed-level call."""
    N, lay = P["N"], soft_batch_layout(OC.soft_qp(P, True))
    sz = lay["sizes"]
    R = len(sets)
    b, q = np.zeros((R, N + 1, 16)), np.zeros((R, N + 1, 16))
    d, z = np.zeros((R, sz["d"])), np.zeros((R, sz["Z"]))
    for r, S in enumerate(sets):
        for k in range(N + 1):
            nu, nx, nb, ns, pnb, pns = sizes(P, k)
            if k < N:
                b[r, k, :P["nx"][k + 1]] = S["b"][k]
            q[r, k, :nu + nx] = _grad(P, S, k)
            oD, oZ = int(lay["oD"][k]), int(lay["oZ"][k])
            lb, ub, zz = np.asarray(S["lb"][k]), np.asarray(S["ub"][k]), np.asarray(S["z"][k])
            d[r, oD:oD + nb], d[r, oD + pnb:oD + pnb + nb] = lb[:nb], ub[:nb]
            d[r, oD + 2 * pnb:oD + 2 * pnb + ns] = lb[nb:]
            d[r, oD + 2 * pnb + pns:oD + 2 * pnb + pns + ns] = ub[nb:]
            z[r, oZ:oZ + ns], z[r, oZ + pns:oZ + pns + ns] = zz[:ns], zz[ns:]
    return b, q, d, z


def packed_iterate(P, v):
    """A per-stage padded list (lam or t) -> the packed (sC,) vector."""
    return np.concatenate([np.asarray(a, dtype=np.float64) for a in v]) if v else np.zeros(0)


def unpack_padded(P, ux, pi, lam, t):
    """One set's padded outputs (ux, pi (N+1, 16); lam, t (sC,)) -> per-stage lists as rel_errors takes them."""
    lay = soft_batch_layout(OC.soft_qp(P, True))
    out = dict(ux=[], pi=[], lam=[], t=[])
    for k in range(P["N"] + 1):
        _, _, _, _, pnb, pns = sizes(P, k)
        out["ux"].append(ux[k])
        if k < P["N"]:
            out["pi"].append(pi[k])
        o, n = int(lay["oC"][k]), 2 * pnb + 4 * pns
        out["lam"].append(lam[o:o + n])
        out["t"].append(t[o:o + n])
    return out


def compact_to_padded(P, blocks):
    """Per-stage compact [lo nb | up nb | 4 x ns] blocks -> per-stage padded lists."""
    out = []
    for k, v in enumerate(blocks):
        _, _, _, _, pnb, pns = sizes(P, k)
        a = np.zeros(2 * pnb + 4 * pns)
        a[live_slots(P, k)] = v
        out.append(a)
    return out

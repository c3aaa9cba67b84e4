"""Soft-constrained MPC problems for d_ip2_mpc_soft_tv (mpc_solvers/d_ip2_soft.c:83-547).

Data contract of the reference (test_problems/test_d_ip_soft.c:277-640):

* ``idxb[k]`` lists the nb[k] hard boxes followed by the ns[k] soft boxes;
* ``d[k]`` = [lb (pnb) | ub (pnb) | ls (pns) | us (pns)] (no general constraints);
* ``Z[k]``, ``z[k]`` = quadratic / linear slack penalties [lower (pns) | upper (pns)];
* ``lam[k]``, ``t[k]`` = [lower (pnb) | upper (pnb) | 4 soft blocks of pns]; ``nu[N] = 0``.
"""
from __future__ import annotations

from dataclasses import dataclass, field

import numpy as np

from .bindings import check, lib, plan_args
from .device import DeviceSolver
from .ocp import mass_spring_dynamics, pack_lib4_batch, rup


@dataclass
class SoftQP:
    N: int
    nx: np.ndarray
    nu: np.ndarray
    nb: np.ndarray
    ns: np.ndarray
    idxb: list
    BAbt: list
    RSQrq: list
    d: list
    Z: list
    z: list
    ng: np.ndarray = field(default=None)
    DCt: list = field(default_factory=list)

    def __post_init__(self):
        if self.ng is None:
            self.ng = np.zeros(self.N + 1, dtype=np.int32)

    def nux(self, k: int) -> int:
        return int(self.nu[k] + self.nx[k])

    def ncv(self, k: int) -> int:
        """length of lam[k] / t[k]: [lower, upper (pnb) | general lower, upper (png) | 4 soft blocks (pns)]"""
        return 2 * rup(int(self.nb[k]), 4) + 2 * rup(int(self.ng[k]), 4) + 4 * rup(int(self.ns[k]), 4)

    def copy(self) -> "SoftQP":
        cp = lambda L: [np.array(a, copy=True) for a in L]
        return SoftQP(self.N, self.nx.copy(), self.nu.copy(), self.nb.copy(), self.ns.copy(), cp(self.idxb),
                      cp(self.BAbt), cp(self.RSQrq), cp(self.d), cp(self.Z), cp(self.z), self.ng.copy(), cp(self.DCt))

    @staticmethod
    def from_case(case) -> "SoftQP":
        """SoftQP of a golden case of kind "soft" (tests/golden/make_golden.py soft)."""
        q = case.qp
        ns = np.asarray(case.inp["ns"][0], dtype=np.float64).astype(np.int32)
        return SoftQP(q.N, q.nx.copy(), q.nu.copy(), q.nb.copy(), ns, [a.copy() for a in q.idxb],
                      [a.copy() for a in q.BAbt], [a.copy() for a in q.RSQrq], [a.copy() for a in q.d],
                      [a.copy() for a in case.inp["Z"]], [a.copy() for a in case.inp["z"]], q.ng.copy(),
                      [a.copy() for a in q.DCt])

    def alloc_solution(self):
        N = self.N
        ux = [np.zeros(rup(self.nux(k) + 1, 4) + 4) for k in range(N + 1)]
        pi = [np.zeros(rup(int(self.nx[k + 1]), 4) + 4) for k in range(N)]
        lam = [np.zeros(self.ncv(k) + 4) for k in range(N + 1)]
        t = [np.zeros(self.ncv(k) + 4) for k in range(N + 1)]
        return ux, pi, lam, t


def mass_spring_soft(N: int, nx: int, nu: int, *, x0=None, Zq: float = 0.0, zl: float = 100.0, Q_diag: float = 0.0,
                     soft_bounds=(-1.0, 1.0), hard_u=(-0.5, 0.5), time_variant: bool = False, seed: int = 0,
                     hard_last: int = 0, soft: bool = True, hard: bool = True) -> SoftQP:
    """The reference's soft-constraint driver problem (test_d_ip_soft.c:160-640): mass-spring dynamics, b = 0,
    x0 = [3.5, 3.5, 0, ...], Q = Q_diag I (0 in the driver), R = 2 I, q = 0.1, r = 0.2; hard input boxes at
    stages 0..N-1 (nb = nu), soft state boxes at stages 1..N (ns = nx), Z = Zq, z = zl.
    ``soft`` / ``hard`` = False drop the soft / hard boxes.
    ``hard_last`` > 0 puts hard boxes on the first ``hard_last`` states of the terminal stage and soft ones on
    the others (a shape the driver does not use: it exercises the reference's soft-gradient index for nb > 0
    at k = N, whose write lands in Zl / zl of stage 1)."""
    A, B = mass_spring_dynamics(nx, nu)
    rng = np.random.Generator(np.random.PCG64(seed))
    if x0 is None:
        x0 = np.zeros(nx)
        x0[0] = x0[1] = 3.5
    b = np.zeros(nx)
    R = 2.0 * np.eye(nu)
    q = np.full(nx, 0.1)
    r = np.full(nu, 0.2)
    nxv = np.array([0] + [nx] * N, dtype=np.int32)
    nuv = np.array([nu] * N + [0], dtype=np.int32)
    nbv = np.array([nu if hard else 0] * N + [hard_last], dtype=np.int32)
    nsv = np.array([0] + [nx if soft else 0] * (N - 1) + [(nx - hard_last) if soft else 0], dtype=np.int32)
    BAbt, RSQrq, dv, idxb, Zv, zv = [], [], [], [], [], []
    for k in range(N + 1):
        nuk, nxk = int(nuv[k]), int(nxv[k])
        nux = nuk + nxk
        if k < N:
            Ak, Bk = A, B
            if time_variant:
                Ak = A + 1e-3 * rng.standard_normal(A.shape)
                Bk = B + 1e-3 * rng.standard_normal(B.shape)
            M = np.zeros((nux + 1, nx))
            M[:nuk, :] = Bk.T
            if k == 0:
                M[nuk, :] = Ak @ x0 + b
            else:
                M[nuk:nux, :] = Ak.T
                M[nux, :] = b
            BAbt.append(pack_lib4_batch(M[None])[0].copy())
        M = np.zeros((nux + 1, nux))
        M[:nuk, :nuk] = R[:nuk, :nuk]
        M[nuk:nux, nuk:nux] = Q_diag * np.eye(nxk)
        M[nux, :nuk] = r[:nuk]
        M[nux, nuk:nux] = q[:nxk]
        RSQrq.append(pack_lib4_batch(M[None])[0].copy())
        nbk, nsk = int(nbv[k]), int(nsv[k])
        pnb, pns = rup(nbk, 4), rup(nsk, 4)
        ib = list(range(min(nuk, nbk))) + [nuk + j for j in range(nbk - min(nuk, nbk))]
        ib += [nuk + nxk - nsk + j for j in range(nsk)]  # soft boxes on the last nsk states (no variable twice)
        idxb.append(np.array(ib, dtype=np.int32) if ib else np.zeros(1, dtype=np.int32))
        dk = np.zeros(2 * pnb + 2 * pns + 4)
        for j in range(nbk):
            lo, hi = hard_u if ib[j] < nuk else (-4.0, 4.0)
            dk[j], dk[pnb + j] = lo, hi
        for j in range(nsk):
            dk[2 * pnb + j], dk[2 * pnb + pns + j] = soft_bounds
        dv.append(dk)
        Zk = np.zeros(2 * pns + 4)
        zk = np.zeros(2 * pns + 4)
        Zk[:nsk] = Zq
        Zk[pns:pns + nsk] = Zq
        zk[:nsk] = zl
        zk[pns:pns + nsk] = zl
        Zv.append(Zk)
        zv.append(zk)
    return SoftQP(N, nxv, nuv, nbv, nsv, idxb, BAbt, RSQrq, dv, Zv, zv)


def random_soft_qp(N: int, nx, nu, nb, ns, *, seed: int, structure_seed: int = 0, x0_scale: float = 2.0,
                   Zq: float = 0.5, zl: float = 10.0) -> SoftQP:
    """Random soft-constrained QP with per-stage sizes (lists of length N + 1; nu[N] is forced to 0): what
    mass_spring_soft fixes is drawn here.
    ``idxb[k]``: nb[k] + ns[k] distinct variables of the nu + nx, drawn by ``structure_seed`` alone (a batch shares
    idxb while its data differ); the hard part and the soft part are each sorted, so the whole is in general not
    monotone, and either part may pick inputs or states.
    Data (``seed``): A = I + 0.1 randn / sqrt(nx) (rectangular where nx changes), B = 0.3 randn, b = 0.05 randn --
    ``x0_scale`` randn on stage 0 when nx[0] = 0, where b stands for A x0; dense SPD stage Hessians G G' / n + I with
    their S block and a gradient 0.5 randn; hard bounds -+(0.5..1.5), soft bounds -+(0.8..1.2); Z = Zq (0.5..1.5)
    and z = zl (0.5..1.5) per element.
    Asserts what the product requires: the tile plan's limits on nb + ns boxes (hpmpc_capi.cpp plan_supported) and
    the b_k read inside BAbt_k (hpmpc_capi_soft.cpp soft_unsupported)."""
    nxv = np.asarray(nx, dtype=np.int32).copy()
    nuv = np.asarray(nu, dtype=np.int32).copy()
    nbv = np.asarray(nb, dtype=np.int32).copy()
    nsv = np.asarray(ns, dtype=np.int32).copy()
    assert N >= 1 and all(len(v) == N + 1 for v in (nxv, nuv, nbv, nsv))
    nuv[N] = 0
    for k in range(N + 1):
        nuk, nxk, nbs = int(nuv[k]), int(nxv[k]), int(nbv[k] + nsv[k])
        assert nuk >= 0 and nxk >= 0 and nuk + nxk <= 16 and rup(nuk, 4) + nxk <= 16, (k, "stage beyond the tile")
        assert nbv[k] >= 0 and nsv[k] >= 0 and nbs <= nuk + nxk and rup(nbs, 4) <= 16, (k, "boxes beyond the plan")
        if k < N and nxv[k + 1] > 0:  # b_k is read with the reference's stride round_up(nx', 4) (d_ip2_soft.c:172)
            nux, nx1 = nuk + nxk, int(nxv[k + 1])
            assert (nux // 4) * 4 * rup(nx1, 4) + nux % 4 + 4 * (nx1 - 1) < rup(nux + 1, 4) * rup(nx1, 2), \
                (k, "b_k read outside BAbt_k")
    srng = np.random.Generator(np.random.PCG64(structure_seed))
    rng = np.random.Generator(np.random.PCG64(seed))
    BAbt, RSQrq, dv, idxb, Zv, zv = [], [], [], [], [], []
    for k in range(N + 1):
        nuk, nxk, nbk, nsk = int(nuv[k]), int(nxv[k]), int(nbv[k]), int(nsv[k])
        nux = nuk + nxk
        pick = srng.permutation(nux)[:nbk + nsk]
        ib = np.concatenate([np.sort(pick[:nbk]), np.sort(pick[nbk:])]).astype(np.int32)
        idxb.append(ib if ib.size else np.zeros(1, dtype=np.int32))
        if k < N:
            nx1 = int(nxv[k + 1])
            M = np.zeros((nux + 1, nx1))
            M[:nuk] = 0.3 * rng.standard_normal((nuk, nx1))
            M[nuk:nux] = (np.eye(nx1, nxk) + 0.1 * rng.standard_normal((nx1, nxk)) / np.sqrt(max(nxk, 1))).T
            M[nux] = (x0_scale if k == 0 and nxk == 0 else 0.05) * rng.standard_normal(nx1)
            BAbt.append(pack_lib4_batch(M[None])[0].copy())
        G = rng.standard_normal((nux, nux))
        M = np.zeros((nux + 1, nux))
        M[:nux] = G @ G.T / max(nux, 1) + np.eye(nux)
        M[nux] = 0.5 * rng.standard_normal(nux)
        RSQrq.append(pack_lib4_batch(M[None])[0].copy())
        pnb, pns = rup(nbk, 4), rup(nsk, 4)
        dk = np.zeros(2 * pnb + 2 * pns + 4)
        dk[:nbk] = -(0.5 + rng.random(nbk))
        dk[pnb:pnb + nbk] = 0.5 + rng.random(nbk)
        dk[2 * pnb:2 * pnb + nsk] = -(0.8 + 0.4 * rng.random(nsk))
        dk[2 * pnb + pns:2 * pnb + pns + nsk] = 0.8 + 0.4 * rng.random(nsk)
        dv.append(dk)
        Zk, zk = np.zeros(2 * pns + 4), np.zeros(2 * pns + 4)
        for o in (0, pns):
            Zk[o:o + nsk] = Zq * (0.5 + rng.random(nsk))
            zk[o:o + nsk] = zl * (0.5 + rng.random(nsk))
        Zv.append(Zk)
        zv.append(zk)
    return SoftQP(N, nxv, nuv, nbv, nsv, idxb, BAbt, RSQrq, dv, Zv, zv)


# ------------------------------------------------------------------------------------------------
# Batched, device-resident soft-constraint IPM (hpmpc_mi355x_ipm_soft_batch, include/hpmpc_mi355x.h): a batch is
# a list of SoftQPs that share stage sizes and idxb.  Problem-major arrays, every stage in the reference's layout:
#   BAbt  (P, packB)  lib4 blocks, stage k at offB[k]        RSQrq (P, packR)  stage k at offR[k]
#   d     (P, sD)     [lb pnb | ub pnb | ls pns | us pns] at oD[k]
#   Z, z  (P, sZ)     [lower pns | upper pns] at oZ[k]
#   lam,t (P, sC)     [lo pnb | up pnb | 4 x pns] at oC[k]
#   ux,pi (P, N+1, 16)
# ------------------------------------------------------------------------------------------------
FSTRIDE = 352  # factor doubles per stage (hpmpc_amd/csrc/hpmpc_kargs.h)


def soft_batch_layout(sq: SoftQP) -> dict:
    """Per-stage offsets oD / oZ / oC (doubles inside one problem's d, Z / z, lam / t) and the per-problem sizes
    (d, Z, C, ux, ws, N) of the batched soft IPM: what hpmpc_mi355x_soft_offsets / _sizes return.  Pure."""
    N = sq.N
    oD, oZ, oC = (np.zeros(N + 1, dtype=np.int64) for _ in range(3))
    sD = sZ = sC = F = padM = 0
    for k in range(N + 1):
        pnb, pns = rup(int(sq.nb[k]), 4), rup(int(sq.ns[k]), 4)
        oD[k], oZ[k], oC[k] = sD, sZ, sC
        sD += 2 * pnb + 2 * pns
        sZ += 2 * pns
        sC += 2 * pnb + 4 * pns
        F += 2 * (pnb + pns) + 4 * pns  # Qx, qx of every stage, then Zl, zl of every stage
        padM = max(padM, 2 * (pnb + pns))
    n1 = N + 1
    # workspace: factor | 7 vectors of 16 per stage | dt dlam lamt tinv | flat block (reference padding) | scal | ist
    ws = n1 * FSTRIDE + 7 * n1 * 16 + 4 * rup(sC + 1, 8) + rup(F + padM + 16, 8) + 8 + 8
    return dict(oD=oD, oZ=oZ, oC=oC, sizes=dict(d=sD, Z=sZ, C=sC, ux=n1 * 16, ws=rup(ws, 32), N=N))


def _same_shape(sqs):
    t = sqs[0]
    for s in sqs[1:]:
        ok = s.N == t.N and all(np.array_equal(getattr(s, f), getattr(t, f)) for f in ("nx", "nu", "nb", "ns", "ng"))
        ok = ok and all(np.array_equal(a[:int(t.nb[k] + t.ns[k])], b[:int(t.nb[k] + t.ns[k])])
                        for k, (a, b) in enumerate(zip(s.idxb, t.idxb)))
        if not ok:
            raise ValueError("the problems of a batch share stage sizes and idxb")


def pack_soft_batch(sqs) -> dict:
    """Problem-major host arrays of a list of SoftQPs (shared sizes and idxb): BAbt, RSQrq, d, Z, z, the stage
    offsets offB / offR of the lib4 blocks and the soft layout (soft_batch_layout)."""
    _same_shape(sqs)
    t = sqs[0]
    N, P = t.N, len(sqs)
    lay = soft_batch_layout(t)
    sz = lay["sizes"]
    offB = np.concatenate([[0], np.cumsum([t.BAbt[k].size for k in range(N)])]).astype(np.int64)
    offR = np.concatenate([[0], np.cumsum([t.RSQrq[k].size for k in range(N + 1)])]).astype(np.int64)
    hB = np.stack([np.concatenate([np.asarray(s.BAbt[k], dtype=np.float64).ravel() for k in range(N)]) for s in sqs])
    hR = np.stack([np.concatenate([np.asarray(s.RSQrq[k], dtype=np.float64).ravel() for k in range(N + 1)])
                   for s in sqs])
    hd, hZ, hz = np.zeros((P, sz["d"])), np.zeros((P, sz["Z"])), np.zeros((P, sz["Z"]))
    for p, s in enumerate(sqs):
        for k in range(N + 1):
            pnb, pns = rup(int(t.nb[k]), 4), rup(int(t.ns[k]), 4)
            n = 2 * pnb + 2 * pns
            hd[p, lay["oD"][k]:lay["oD"][k] + n] = s.d[k][:n]
            hZ[p, lay["oZ"][k]:lay["oZ"][k] + 2 * pns] = s.Z[k][:2 * pns]
            hz[p, lay["oZ"][k]:lay["oZ"][k] + 2 * pns] = s.z[k][:2 * pns]
    return dict(BAbt=hB, RSQrq=hR, d=hd, Z=hZ, z=hz, offB=offB[:N], offR=offR[:N + 1], packB=int(offB[-1]),
                packR=int(offR[-1]), layout=lay)


def unpack_soft_batch(template: SoftQP, packed: dict) -> list:
    """Inverse of pack_soft_batch: the SoftQPs whose sizes / idxb are the template's and whose data are the packed
    arrays (the vectors keep the template's padded lengths; the padding is zero)."""
    N, lay = template.N, packed["layout"]
    out = []
    for p in range(packed["BAbt"].shape[0]):
        s = template.copy()
        for k in range(N + 1):
            if k < N:
                s.BAbt[k] = packed["BAbt"][p, packed["offB"][k]:packed["offB"][k] + template.BAbt[k].size].copy()
            s.RSQrq[k] = packed["RSQrq"][p, packed["offR"][k]:packed["offR"][k] + template.RSQrq[k].size].copy()
            pnb, pns = rup(int(template.nb[k]), 4), rup(int(template.ns[k]), 4)
            n = 2 * pnb + 2 * pns
            s.d[k] = np.zeros_like(template.d[k])
            s.d[k][:n] = packed["d"][p, lay["oD"][k]:lay["oD"][k] + n]
            s.Z[k] = np.zeros_like(template.Z[k])
            s.z[k] = np.zeros_like(template.z[k])
            s.Z[k][:2 * pns] = packed["Z"][p, lay["oZ"][k]:lay["oZ"][k] + 2 * pns]
            s.z[k][:2 * pns] = packed["z"][p, lay["oZ"][k]:lay["oZ"][k] + 2 * pns]
        out.append(s)
    return out


def unpack_soft_solution(template: SoftQP, ux, pi, lam, t, kk, ret, stat) -> list:
    """Per-problem results of a batched solve, shaped like HpmpcAPI.ipm_soft's: dicts of ret, kk, stat (5 kk) and the
    per-stage lists ux (nu + nx), pi (nx[k+1]), lam / t (2 pnb + 4 pns).  Arrays: host (numpy) copies of the
    solver's ux / pi (P, N+1, 16), lam / t (P, sC), kk / ret (P), stat (P, 5 k_max)."""
    N, lay = template.N, soft_batch_layout(template)
    out = []
    for p in range(len(kk)):
        k_it = int(kk[p])
        r = dict(ret=int(ret[p]), kk=k_it, stat=np.array(stat[p, :5 * max(k_it, 0)], copy=True), ux=[], pi=[], lam=[],
                 t=[])
        for k in range(N + 1):
            r["ux"].append(np.array(ux[p, k, :template.nux(k)], copy=True))
            if k < N:
                r["pi"].append(np.array(pi[p, k, :int(template.nx[k + 1])], copy=True))
            o, n = int(lay["oC"][k]), template.ncv(k)
            r["lam"].append(np.array(lam[p, o:o + n], copy=True))
            r["t"].append(np.array(t[p, o:o + n], copy=True))
        out.append(r)
    return out


_soft_lib = lib  # the soft calls are bound with every other one (hpmpc_amd.bindings)


def soft_plan_create(sq: SoftQP):
    """hpmpc_mi355x_soft_plan_create on a SoftQP's sizes.  Returns (plan or None, last error code)."""
    L = lib()
    (nx, nu, nb, ng, ns), idxp, _keep = plan_args(sq.idxb, sq.nx, sq.nu, sq.nb, sq.ng, sq.ns)
    plan = L.hpmpc_mi355x_soft_plan_create(sq.N, nx, nu, nb, idxp, ng, ns)
    return (plan or None), int(L.hpmpc_mi355x_last_error())


class SoftBatchSolver(DeviceSolver):
    """Device-resident batch of soft-constrained QPs + hpmpc_mi355x_ipm_soft_batch: every iteration of every problem
    in one launch on torch's current stream (torch is plumbing: allocation and streams).  There is no CPU fallback.

    ``shared=True`` keeps one copy of the BAbt / RSQrq blocks of stages >= 1 for the whole batch (they must be equal
    in every problem) and stage 0 per problem, through hpmpc_mi355x_layout's shared flags."""

    _destroy = "hpmpc_mi355x_soft_plan_destroy"

    def __init__(self, sqs, k_max: int = 50, device="cuda", shared: bool = False):
        import ctypes as C

        from .batch import _Layout

        super().__init__(device)
        torch = self.torch
        self.sqs = list(sqs)
        self.template = t = self.sqs[0]
        self.N, self.nprob, self.k_max = t.N, len(self.sqs), int(k_max)
        L = lib()
        pk = pack_soft_batch(self.sqs)
        self.plan, err = soft_plan_create(t)
        if not self.plan:
            raise ValueError(f"unsupported problem for the batched soft IPM (code {err})")
        sz = (C.c_longlong * 6)()
        L.hpmpc_mi355x_soft_sizes(self.plan, sz)
        self.sizes = dict(zip(("d", "Z", "C", "ux", "ws", "N"), (int(v) for v in sz)))
        off = (C.c_longlong * (3 * (self.N + 1)))()
        L.hpmpc_mi355x_soft_offsets(self.plan, off)
        self.offsets = np.array(off[:], dtype=np.int64).reshape(self.N + 1, 3)  # oD oZ oC
        N, P, f64 = self.N, self.nprob, torch.float64
        hB, hR, offB, offR = pk["BAbt"], pk["RSQrq"], pk["offB"].copy(), pk["offR"].copy()
        sB, sR, shB, shR = pk["packB"], pk["packR"], None, None
        if shared:
            if not ((hB[:, offB[1] if N > 1 else sB:] == hB[:1, offB[1] if N > 1 else sB:]).all()
                    and (hR[:, offR[1]:] == hR[:1, offR[1]:]).all()):
                raise ValueError("stage data beyond stage 0 differ between problems")
            b0, r0 = int(offB[1]) if N > 1 else sB, int(offR[1])
            # [blocks of stages >= 1, once | stage 0 of problem 0 | stage 0 of problem 1 | ...]
            offB = np.array([sB - b0] + [int(o) - b0 for o in offB[1:]], dtype=np.int64)
            offR = np.array([sR - r0] + [int(o) - r0 for o in offR[1:]], dtype=np.int64)
            hB = np.concatenate([hB[0, b0:], hB[:, :b0].reshape(-1)])
            hR = np.concatenate([hR[0, r0:], hR[:, :r0].reshape(-1)])
            sB, sR = b0, r0
            shB = np.array([0] + [1] * (N - 1), dtype=np.uint8)
            shR = np.array([0] + [1] * N, dtype=np.uint8)
        self._keep = (offB, offR, shB, shR)
        ll, u8 = C.POINTER(C.c_longlong), C.POINTER(C.c_ubyte)
        self.layout = _Layout(sB, sR, offB.ctypes.data_as(ll), offR.ctypes.data_as(ll),
                              shB.ctypes.data_as(u8) if shared else None, shR.ctypes.data_as(u8) if shared else None)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)
        self.BAbt, self.RSQrq = up(hB), up(hR)
        self.d, self.Z, self.z = up(pk["d"]), up(pk["Z"]), up(pk["z"])
        self.ux = torch.zeros((P, N + 1, 16), dtype=f64, device=self.dev)
        self.pi = torch.zeros((P, N + 1, 16), dtype=f64, device=self.dev)
        self.lam = torch.zeros((P, self.sizes["C"]), dtype=f64, device=self.dev)
        self.t = torch.zeros((P, self.sizes["C"]), dtype=f64, device=self.dev)
        self.ws = torch.empty((P, self.sizes["ws"]), dtype=f64, device=self.dev)  # needs no initialisation
        self.kk = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.ret = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.stat = torch.zeros((P, 5 * max(self.k_max, 1)), dtype=f64, device=self.dev)

    def set_ux(self, ux0):
        """Warm-start iterate: ux0[p][k] holds at least nu + nx values of problem p, stage k."""
        h = np.zeros((self.nprob, self.N + 1, 16))
        for p in range(self.nprob):
            for k in range(self.N + 1):
                n = self.template.nux(k)
                h[p, k, :n] = np.asarray(ux0[p][k])[:n]
        self.ux.copy_(self.torch.from_numpy(h))

    def solve(self, *, k_max=None, mu0=100.0, mu_tol=1e-8, alpha_min=1e-8, warm_start=0, compute_mult=1, p0=0,
              count=None):
        """Batched d_ip2_mpc_soft_tv on problems [p0, p0 + count), asynchronous on torch's current stream.
        k_max: at most the solver's (its stat rows are 5 k_max wide)."""
        import ctypes as C

        k_max = self.k_max if k_max is None else int(k_max)
        assert 0 <= k_max <= self.k_max
        p0, count = self._range(p0, count)
        # stat keeps the stride the call uses: 5 k_max per problem
        stat = self.stat if k_max == self.k_max else self.stat.view(-1)[:self.nprob * 5 * max(k_max, 1)]
        self._stat_kmax = k_max
        check(lib().hpmpc_mi355x_ipm_soft_batch(
            self.plan, C.byref(self.layout), self.nprob, p0, count, self.BAbt.data_ptr(), self.RSQrq.data_ptr(),
            self.Z.data_ptr(), self.z.data_ptr(), self.d.data_ptr(), self.ux.data_ptr(), self.pi.data_ptr(),
            self.lam.data_ptr(), self.t.data_ptr(), self.ws.data_ptr(), k_max, mu0, mu_tol, alpha_min, warm_start,
            compute_mult, self.kk.data_ptr(), self.ret.data_ptr(), stat.data_ptr(),
            self._stream()), "hpmpc_mi355x_ipm_soft_batch")

    def kkt_buffers(self, nrhs: int = 1) -> dict:
        """The output and scratch tensors kkt_new_rhs(nrhs=nrhs) writes (allocated on first use, then reused): ux, pi
        (nprob, nrhs, N+1, 16), lam, t (nprob, nrhs, sizes["C"]), scratch (nprob, nrhs,
        hpmpc_mi355x_soft_kkt_scratch_doubles)."""
        def make(n):
            new = lambda *shape: self.torch.zeros((self.nprob, n) + shape, dtype=self.torch.float64, device=self.dev)
            return dict(ux=new(self.N + 1, 16), pi=new(self.N + 1, 16), lam=new(self.sizes["C"]),
                        t=new(self.sizes["C"]), scratch=new(int(lib().hpmpc_mi355x_soft_kkt_scratch_doubles(self.plan))))
        return self._per_set("soft_kkt", nrhs, make)

    def kkt_new_rhs(self, b, q, d, z=None, nrhs=1, refactor=True, p0=0, count=None, compute_mult=1, out=None,
                    lam0=None, t0=None):
        """The batched soft KKT re-solve (hpmpc_mi355x_soft_kkt_batch): the affine Newton point of a linearisation for
        ``nrhs`` right-hand-side sets per problem, one Riccati solve each.  b, q: (nprob, nrhs, N+1, 16) device tensors
        (b in state order, q in variable order [r | q]); d: (nprob, nrhs, sizes["d"]); z: (nprob, nrhs, sizes["Z"]) or
        None for the problem's own z.  refactor=True linearises at (lam0, t0) -- default: the solver's iterate lam, t --
        and factorises into ws first; refactor=False reads the linearisation the last iteration of solve() left in ws
        (kk >= 1).  Returns ux, pi (nprob, nrhs, N+1, 16) and lam, t (nprob, nrhs, sizes["C"]): the tensors of ``out``
        (default: kkt_buffers(nrhs), overwritten by the next call).  The problem data and the solver's iterate are not
        written; ws only with refactor.  Asynchronous on torch's current stream."""
        import ctypes as C

        p0, count = self._range(p0, count)
        out = self.kkt_buffers(nrhs) if out is None else out
        P, n1, sz = self.nprob, self.N + 1, self.sizes
        ins = [self._tensor(x, shape, name, opt) for name, x, shape, opt in (
            ("b", b, (P, nrhs, n1, 16), False), ("q", q, (P, nrhs, n1, 16), False), ("d", d, (P, nrhs, sz["d"]), False),
            ("z", z, (P, nrhs, sz["Z"]), True))]
        base = [None, None]
        if refactor:
            base = [self._tensor(self.lam if lam0 is None else lam0, (P, sz["C"]), "lam0"),
                    self._tensor(self.t if t0 is None else t0, (P, sz["C"]), "t0")]
        for name, shape in (("ux", (P, nrhs, n1, 16)), ("pi", (P, nrhs, n1, 16)), ("lam", (P, nrhs, sz["C"])),
                            ("t", (P, nrhs, sz["C"]))):
            self._tensor(out[name], shape, f"out[{name!r}]")
        check(lib().hpmpc_mi355x_soft_kkt_batch(
            self.plan, C.byref(self.layout), P, p0, count, nrhs, self.BAbt.data_ptr(), self.RSQrq.data_ptr(),
            self.Z.data_ptr(), self.z.data_ptr(), *base, *ins, out["ux"].data_ptr(), out["pi"].data_ptr(),
            out["lam"].data_ptr(), out["t"].data_ptr(), self.ws.data_ptr(), out["scratch"].data_ptr(),
            1 if refactor else 0, compute_mult, self._stream()), "hpmpc_mi355x_soft_kkt_batch")
        return out["ux"], out["pi"], out["lam"], out["t"]

    def results(self) -> list:
        """Synchronise and return the per-problem dicts of unpack_soft_solution."""
        self.torch.cuda.synchronize(self.dev)
        k_max = getattr(self, "_stat_kmax", self.k_max)
        stat = self.stat.view(-1)[:self.nprob * 5 * max(k_max, 1)].view(self.nprob, -1).cpu().numpy()
        c = lambda x: x.cpu().numpy()
        return unpack_soft_solution(self.template, c(self.ux), c(self.pi), c(self.lam), c(self.t), c(self.kk),
                                    c(self.ret), stat)


def soft_algorithmic_bytes_per_ip_iter(sq: SoftQP) -> float:
    """Algorithmic HBM bytes of one iteration of one problem through hk_soft_ipm, each datum counted
    once per body, T = nux (nux + 1) / 2:
    - Riccati sv: BAbt with its b row, lower(RSQrq), q, Qx / qx slots read; L lower + row + inv_diag, P b, dux, dpi
      written.  Riccati trs: L, BAbt, b, q, qx slots, P b read; dux, dpi written;
    - constraint passes per hard box pair: hess 16, pred 20, corr 19 doubles; per soft box (four slack blocks):
      hess 34, pred 42, corr 39 (t, lam, dt, dlam, lamt, tinv, d, Z, z, Zl, zl, the Qx / qx slots and their flat twins);
    - corr: ux, dux read and ux written (3 nux), the same for pi (3 nx')."""
    tot = 0
    N = sq.N
    for k in range(N + 1):
        nux = sq.nux(k)
        nx1 = int(sq.nx[k + 1]) if k < N else 0
        nb, ns = int(sq.nb[k]), int(sq.ns[k])
        T = nux * (nux + 1) // 2
        L = T + 2 * nux
        babt = (nux + 1) * nx1
        sv = babt + T + nux + 2 * (nb + ns) + L + nx1 + nux + nx1
        trs = L + babt + (nux + nx1) + (nb + ns) + nx1 + (nux + nx1)
        tot += sv + trs + 55 * nb + 115 * ns + 3 * nux + 3 * nx1
    return 8.0 * tot

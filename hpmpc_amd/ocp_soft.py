"""Batched OCP front end for soft-constrained problems: dense data in HBM -> pack -> the one-launch soft IPM -> the
outputs and residual norms of fortran_order_d_ip_ocp_soft_tv.

``OcpSoftBatchSolver`` is that wrapper's top layer for ``nprob`` problems that share stage sizes and box indices and
whose dense data are torch tensors on the device (hpmpc_mi355x_ocp_soft_* in include/hpmpc_mi355x.h, hk_ocp_soft.hip).
torch is plumbing here (allocation, streams); packing, the solve, the residual and the outputs are HIP kernels.

Dense arrays, per problem: the stage blocks concatenated in stage order -- A, B, b, Q, S, R, q, r as in
hpmpc_amd.ocp_batch; lb_k, ub_k with nb[k] + ns[k] entries (the hard boxes, then the soft ones, in the order of
idxb[k]); Z_k, z_k with 2 ns[k] entries, [lower ns | upper ns].  The outputs u, x, pi have the shapes of r, q, b; lam and
t are compact, [lo nb | up nb | 4 soft blocks of ns] per stage.

The linear penalty z: the reference wrapper never copies z into the IPM and solves with z = 0.  Here a missing "z"
packs zeros (the wrapper's behaviour) and a given one is used -- a documented extension (include/hpmpc_mi355x.h).
The host-side helpers below need numpy only (no library load).
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .bindings import check, lib, plan_args
from .device import DeviceSolver
from .ocp import rup, unpack_lib4

KEYS = ("A", "B", "b", "Q", "S", "R", "q", "r", "lb", "ub", "Z", "z")  # hpmpc_mi355x_ocp_soft_data
OUT_KEYS = ("u", "x", "pi", "lam", "t")
NSIZES, NOFFSETS = 27, 18  # HPMPC_MI355X_OCP_SOFT_NSIZES / _NOFFSETS
# indices into hpmpc_mi355x_ocp_soft_sizes beyond the 12 dense arrays
SZ = dict(BAbt=12, RSQrq=13, d=14, Zp=15, ux=16, lam=17, ws=18, res=19, u=20, x=21, pi_out=22, lam_out=23,
          inf_norm_res=24, res_ok=25, N=26)


def soft_iface_from_qp(sq) -> dict:
    """SoftQP (hpmpc_amd.soft) -> the interface form of oracle/iface_oracle.py with ns, Z and z: the inverse of
    to_soft_qp, which reproduces BAbt, RSQrq, d, Z and idxb of ``sq`` bit for bit (z is kept too; to_soft_qp drops it
    as the reference wrapper does).  RSQrq_k must hold S in both triangles."""
    N = sq.N
    nx, nu = [int(v) for v in sq.nx], [int(v) for v in sq.nu]
    nb, ns = [int(v) for v in sq.nb], [int(v) for v in sq.ns]
    P = dict(N=N, nx=nx, nu=nu, nb=nb, ns=ns, ng=[0] * (N + 1), A=[], B=[], b=[], Q=[], S=[], R=[], q=[], r=[], lb=[],
             ub=[], hidxb=[], Z=[], z=[], C=[], D=[], lg=[], ug=[])
    for k in range(N + 1):
        nuk, nxk, nux = nu[k], nx[k], nu[k] + nx[k]
        if k < N:
            M = np.array(unpack_lib4(sq.BAbt[k], nux + 1, nx[k + 1]))
            P["B"].append(M[:nuk].T.copy())
            P["A"].append(M[nuk:nux].T.copy())
            P["b"].append(M[nux].copy())
        M = np.array(unpack_lib4(sq.RSQrq[k], nux + 1, nux))
        P["R"].append(M[:nuk, :nuk].copy())
        P["S"].append(M[:nuk, nuk:nux].copy())
        P["Q"].append(M[nuk:nux, nuk:nux].copy())
        P["r"].append(M[nux, :nuk].copy())
        P["q"].append(M[nux, nuk:nux].copy())
        pnb, pns = rup(nb[k], 4), rup(ns[k], 4)
        d, o = np.asarray(sq.d[k], dtype=np.float64), 2 * pnb
        P["lb"].append(np.r_[d[:nb[k]], d[o:o + ns[k]]])
        P["ub"].append(np.r_[d[pnb:pnb + nb[k]], d[o + pns:o + pns + ns[k]]])
        for key, v in (("Z", sq.Z[k]), ("z", sq.z[k])):
            P[key].append(np.r_[v[:ns[k]], v[pns:pns + ns[k]]].astype(np.float64))
        P["hidxb"].append(np.array(sq.idxb[k], dtype=np.int32, copy=True))
        P["C"].append(np.zeros((0, nxk)))
        P["D"].append(np.zeros((0, nuk)))
        P["lg"].append(np.zeros(0))
        P["ug"].append(np.zeros(0))
    return P


def _shape(key, N, nx, nu, nb, ns, k):
    """Shape of stage k's block of a dense or output array (a stage without the block has a zero dimension)."""
    nuk = int(nu[k]) if k < N else 0
    nxk, nbk, nsk = int(nx[k]), int(nb[k]), int(ns[k])
    nx1 = int(nx[k + 1]) if k < N else 0
    return {"A": (nx1, nxk), "B": (nx1, nuk), "b": (nx1,), "Q": (nxk, nxk), "S": (nuk, nxk), "R": (nuk, nuk),
            "q": (nxk,), "r": (nuk,), "lb": (nbk + nsk,), "ub": (nbk + nsk,), "Z": (2 * nsk,), "z": (2 * nsk,),
            "u": (nuk,), "x": (nxk,), "pi": (nx1,), "lam": (2 * nbk + 4 * nsk,), "t": (2 * nbk + 4 * nsk,)}[key]


def soft_dense_layout(N, nx, nu, nb, ns) -> dict:
    """Doubles per problem (``sizes[key]``) and per-stage offsets (``offsets[key]``, N+1 entries) of every dense array
    and of the outputs u, x, pi, lam, t: the formulas of hpmpc_mi355x_ocp_soft_sizes / _offsets."""
    sizes, offsets = {}, {}
    for key in KEYS + OUT_KEYS:
        off, o = np.zeros(N + 1, dtype=np.int64), 0
        for k in range(N + 1):
            off[k] = o
            o += int(np.prod(_shape(key, N, nx, nu, nb, ns, k)))
        sizes[key], offsets[key] = o, off
    return dict(sizes=sizes, offsets=offsets)


def _sizes_of(P):
    return P["N"], list(P["nx"]), list(P["nu"]), list(P["nb"]), list(P["ns"])


def flatten_soft_problems(problems, order="C", keys=KEYS) -> dict:
    """Interface-form soft problems (same sizes) -> {key: (nprob, size) float64}: each problem's stage blocks flattened
    in ``order`` ("C" row-major, "F" column-major) and concatenated in stage order."""
    N, nx, nu, nb, ns = _sizes_of(problems[0])
    lay = soft_dense_layout(N, nx, nu, nb, ns)
    out = {}
    for key in keys:
        arr = np.zeros((len(problems), lay["sizes"][key]))
        for p, P in enumerate(problems):
            if _sizes_of(P) != (N, nx, nu, nb, ns):
                raise ValueError("the problems of a batch share their stage sizes")
            for k, M in enumerate(P[key]):
                M = np.asarray(M, dtype=np.float64)
                shp = _shape(key, N, nx, nu, nb, ns, k)
                if M.size != int(np.prod(shp)):
                    raise ValueError(f"{key}[{k}] has {M.size} entries, expected shape {shp}")
                o = lay["offsets"][key][k]
                arr[p, o:o + M.size] = M.reshape(shp).flatten(order)
        out[key] = arr
    return out


def unflatten_soft_outputs(flat, N, nx, nu, nb, ns, keys=OUT_KEYS) -> list:
    """{key: (nprob, size)} of the outputs u, x, pi, lam, t -> one dict per problem of per-stage blocks (u and pi get
    N blocks, the others N+1)."""
    lay = soft_dense_layout(N, nx, nu, nb, ns)
    out = []
    for p in range(len(np.asarray(flat[keys[0]]))):
        P = {}
        for key in keys:
            row = np.asarray(flat[key])[p]
            blocks = []
            for k in range(N if key in ("u", "pi") else N + 1):
                n, o = _shape(key, N, nx, nu, nb, ns, k)[0], lay["offsets"][key][k]
                blocks.append(row[o:o + n].copy())
            P[key] = blocks
        out.append(P)
    return out


SET_KEYS = ("b", "q", "r", "lb", "ub", "z")  # the per-set vectors of hpmpc_mi355x_soft_kkt_ocp_batch


def flatten_soft_sets(sets, order="C", keys=SET_KEYS) -> dict:
    """Per-set vectors of the soft re-solve: ``sets[p][r]`` is an interface-form dict (at least the sizes and ``keys``)
    of problem p's set r -> {key: (nprob, nrhs, size) float64}, each set flattened as flatten_soft_problems does."""
    per = [flatten_soft_problems(row, order, keys) for row in sets]
    return {key: np.stack([f[key] for f in per]) for key in keys}


def unflatten_soft_set_outputs(flat, N, nx, nu, nb, ns, keys=OUT_KEYS) -> list:
    """{key: (nprob, nrhs, size)} of the per-set outputs u, x, pi, lam, t -> ``out[p][r]``: the per-stage blocks of
    problem p's set r, as unflatten_soft_outputs gives them per problem."""
    nprob = len(np.asarray(flat[keys[0]]))
    return [unflatten_soft_outputs({k: np.asarray(flat[k])[p] for k in keys}, N, nx, nu, nb, ns, keys)
            for p in range(nprob)]


class _OcpSoftData(C.Structure):
    _fields_ = [("ptr", C.c_void_p * len(KEYS)), ("stride", C.c_longlong * len(KEYS))]


def ocp_soft_plan_create(N, nx, nu, nb, idxb, ns, ng=None, order="C"):
    """(plan handle or None, error code, keep-alive objects) of hpmpc_mi355x_ocp_soft_plan_create."""
    L = lib()
    nuv = list(nu) + [0] * (N + 1 - len(nu))
    ng = [0] * (N + 1) if ng is None else ng
    (pnx, pnu, pnb, png, pns), idxp, keep = plan_args(idxb, nx, nuv, nb, ng, ns)
    plan = L.hpmpc_mi355x_ocp_soft_plan_create(N, pnx, pnu, pnb, idxp, png, pns, 1 if order == "C" else 0)
    return (plan or None), L.hpmpc_mi355x_last_error(), keep


class OcpSoftBatchSolver(DeviceSolver):
    """``nprob`` soft-constrained OCPs with the given stage sizes and the dense device tensors ``data``: {key: tensor
    (nprob, size), or (size,) for an array shared by every problem (stride 0)} over A, B, b, Q, S, R, q, r, lb, ub, Z
    and optionally z.  Owns the packed arrays, the iterate, the workspace and the outputs.  pack() -> solve() ->
    finish(), all asynchronous on torch's current stream; for a receding-horizon step overwrite the data tensors (or
    pass new ones to pack) and pack(matrices=False).
    There is no CPU fallback: without a GPU or the built library the constructor raises."""

    _destroy = "hpmpc_mi355x_ocp_soft_plan_destroy"

    def __init__(self, N, nx, nu, nb, idxb, ns, data, nprob=None, order="C", device="cuda", k_max=50):
        if order not in ("C", "F"):
            raise ValueError("order is 'C' (row-major blocks) or 'F' (column-major blocks)")
        super().__init__(device)
        torch = self.torch
        self.N, self.k_max, self.order = int(N), int(k_max), order
        self.nx, self.nu = [int(v) for v in nx], [int(v) for v in nu][:N] + [0]
        self.nb, self.ns = [int(v) for v in nb], [int(v) for v in ns]
        if nprob is None:
            rows = {int(x.shape[0]) for x in data.values() if x is not None and x.dim() == 2}
            if len(rows) != 1:
                raise ValueError("nprob: give it, or one (nprob, size) tensor at least (and no two that differ)")
            nprob = rows.pop()
        self.nprob = int(nprob)
        L = lib()
        self.plan, err, self._keep = ocp_soft_plan_create(N, self.nx, self.nu, self.nb, idxb, self.ns, order=order)
        if not self.plan:
            raise ValueError(f"unsupported problem sizes for the soft OCP front end (code {err})")
        sz = np.zeros(NSIZES, dtype=np.int64)
        L.hpmpc_mi355x_ocp_soft_sizes(self.plan, sz.ctypes.data)
        self.sizes = {k: int(sz[i]) for i, k in enumerate(KEYS)}
        self.sizes.update({k: int(sz[i]) for k, i in SZ.items()})
        self.res_ok = bool(self.sizes["res_ok"])
        off = np.zeros((N + 1, NOFFSETS), dtype=np.int64)
        L.hpmpc_mi355x_ocp_soft_offsets(self.plan, off.ctypes.data)
        self.offsets = {k: off[:, i].copy() for i, k in enumerate(KEYS)}
        self.offsets.update(lam_out=off[:, 12].copy(), BAbt=off[:, 13].copy(), RSQrq=off[:, 14].copy(),
                            d=off[:, 15].copy(), Zp=off[:, 16].copy(), lam=off[:, 17].copy())
        self.data = dict(data)
        P, s = self.nprob, self.sizes
        new = lambda n, dt=torch.float64: torch.zeros((P, max(n, 1)), dtype=dt, device=self.dev)
        self.BAbt, self.RSQrq, self.d = new(s["BAbt"]), new(s["RSQrq"]), new(s["d"])
        self.Zp, self.zp = new(s["Zp"]), new(s["Zp"])  # the packed Z / z
        self.ux, self.pi, self.lam, self.t = new(s["ux"]), new(s["ux"]), new(s["lam"]), new(s["lam"])
        self.ws = torch.empty((P, s["ws"]), dtype=torch.float64, device=self.dev)  # needs no initialisation
        self.res = new(s["res"])
        self.u, self.x, self.pi_out = new(s["u"]), new(s["x"]), new(s["pi_out"])
        self.lam_out, self.t_out = new(s["lam_out"]), new(s["lam_out"])
        self.inf_norm_res = new(4)
        self.kk = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.ret = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.stat = new(5 * max(self.k_max, 1))

    def _vec(self, x, n, what):
        """(pointer, problem stride) of a float64 device tensor: (nprob, n) with unit inner stride, or (n,) shared by
        every problem (stride 0)."""
        if x.dim() == 2 and x.shape[0] == self.nprob:
            return self._tensor(x[0], (n,), what), x.stride(0)
        return self._tensor(x, (n,), what), 0

    def data_struct(self, data=None):
        """hpmpc_mi355x_ocp_soft_data of the solver's dense tensors (or of ``data``); only z may be missing."""
        data = self.data if data is None else data
        ds = _OcpSoftData()
        for i, key in enumerate(KEYS):
            x = data.get(key)
            if x is None:
                if key != "z" and self.sizes[key]:
                    raise ValueError(f"dense array {key} missing")
                ds.ptr[i], ds.stride[i] = None, 0
            else:
                ds.ptr[i], ds.stride[i] = self._vec(x, self.sizes[key], key)
        return ds

    def _packed(self):
        """The packed BAbt, RSQrq, Z, z, d, in the argument order of the solve and the finish."""
        return tuple(x.data_ptr() for x in (self.BAbt, self.RSQrq, self.Zp, self.zp, self.d))

    def pack(self, matrices=True, warm=None, data=None, p0=0, count=None):
        """Dense device tensors -> BAbt, RSQrq, d, Z, z (hk_ocp_soft_pack).  ``data``: tensors that replace the
        solver's (by key) from this call on.  matrices=False rewrites only b, q, r, the bounds and the penalties.
        warm: {"u": (nprob, sizes["u"]), "x": (nprob, sizes["x"])} packed into ux for warm_start=1."""
        p0, count = self._range(p0, count)
        if data is not None:
            self.data.update(data)
        ds = self.data_struct()
        u0 = x0 = ux = None
        if warm is not None:
            u0 = self._tensor(warm["u"], (self.nprob, self.sizes["u"]), "warm u")
            x0 = self._tensor(warm["x"], (self.nprob, self.sizes["x"]), "warm x")
            ux = self.ux.data_ptr()
        check(lib().hpmpc_mi355x_ocp_soft_pack_batch(
            self.plan, C.byref(ds), 1 if matrices else 0, self.nprob, p0, count, self.BAbt.data_ptr(),
            self.RSQrq.data_ptr(), self.d.data_ptr(), self.Zp.data_ptr(), self.zp.data_ptr(), u0, x0, ux,
            self._stream()), "hpmpc_mi355x_ocp_soft_pack_batch")

    def solve(self, mu0=100.0, mu_tol=1e-8, alpha_min=1e-8, warm_start=0, k_max=None, p0=0, count=None):
        """d_ip2_mpc_soft_tv on the packed batch, every iteration in one launch (mu0 > 0: one value for the batch).
        k_max: at most the solver's (its stat rows are 5 k_max wide)."""
        k_max = self.k_max if k_max is None else int(k_max)
        assert 0 <= k_max <= self.k_max
        p0, count = self._range(p0, count)
        self._stat_kmax = k_max
        check(lib().hpmpc_mi355x_ocp_soft_ipm_batch(
            self.plan, self.nprob, p0, count, *self._packed(), self.ux.data_ptr(), self.pi.data_ptr(),
            self.lam.data_ptr(), self.t.data_ptr(), self.ws.data_ptr(), k_max, mu0, mu_tol, alpha_min, warm_start, 1,
            self.kk.data_ptr(), self.ret.data_ptr(), self.stat.data_ptr(), self._stream()),
            "hpmpc_mi355x_ocp_soft_ipm_batch")

    def _sized(self, o):
        s = self.sizes
        n = dict(u=s["u"], x=s["x"], pi=s["pi_out"], lam=s["lam_out"], t=s["lam_out"])
        return {key: o[key][..., :n[key]] for key in n}

    def finish(self, norms=None, p0=0, count=None) -> dict:
        """The wrapper's outputs as device tensors (nprob, size): u, x, pi, compact lam and t, kk and status per
        problem, and with ``norms`` inf_norm_res (nprob, 4) from the batched d_res_mpc_soft_tv.  norms=None computes
        them iff the plan's res_ok holds (include/hpmpc_mi355x.h); norms=True on a plan with res_ok = 0 raises.
        Asynchronous: synchronise before reading."""
        p0, count = self._range(p0, count)
        norms = self.res_ok if norms is None else bool(norms)
        if norms and not self.res_ok:
            raise ValueError("residual norms: the reference's soft residual reads idxb[k][nu + i] outside idxb[k] on "
                             "these sizes (res_ok = 0)")
        check(lib().hpmpc_mi355x_ocp_soft_finish_batch(
            self.plan, self.nprob, p0, count, *self._packed(), self.ux.data_ptr(), self.pi.data_ptr(),
            self.lam.data_ptr(), self.t.data_ptr(), self.res.data_ptr(), self.u.data_ptr(), self.x.data_ptr(),
            self.pi_out.data_ptr(), self.lam_out.data_ptr(), self.t_out.data_ptr(),
            self.inf_norm_res.data_ptr() if norms else None, self._stream()), "hpmpc_mi355x_ocp_soft_finish_batch")
        out = dict(self._sized(dict(u=self.u, x=self.x, pi=self.pi_out, lam=self.lam_out, t=self.t_out)), kk=self.kk,
                   status=self.ret)
        if norms:
            out["inf_norm_res"] = self.inf_norm_res
        return out

    def kkt_buffers(self, nrhs: int = 1) -> dict:
        """The tensors kkt_sets(nrhs=nrhs) writes (allocated on first use, then reused): the dense outputs u, x, pi, lam,
        t (nprob, nrhs, max(size, 1)), the packed per-set work buffer and the scratch."""
        def make(n):
            s, L = self.sizes, lib()
            new = lambda m: self.torch.zeros((self.nprob, n, max(int(m), 1)), dtype=self.torch.float64, device=self.dev)
            return dict(u=new(s["u"]), x=new(s["x"]), pi=new(s["pi_out"]), lam=new(s["lam_out"]), t=new(s["lam_out"]),
                        work=new(L.hpmpc_mi355x_soft_kkt_ocp_work_doubles(self.plan)),
                        scratch=new(L.hpmpc_mi355x_soft_kkt_scratch_doubles(L.hpmpc_mi355x_ocp_soft_ipm_plan(self.plan))))
        return self._per_set("soft_kkt", nrhs, make)

    def kkt_sets(self, sets, nrhs, refactor=True, p0=0, count=None) -> dict:
        """The batched soft KKT re-solve on dense vectors (hpmpc_mi355x_soft_kkt_ocp_batch): ``nrhs`` right-hand-side
        sets per problem against one linearisation of the packed problems.  ``sets``: {key: contiguous float64 device
        tensor (nprob, nrhs, sizes[key])} over b, q, r, lb, ub and optionally z (missing: every set takes the packed z
        of its problem).  refactor=True linearises at the solver's iterate (lam, t) and factorises into ws first;
        refactor=False reads the linearisation the last iteration of solve() left in ws (kk >= 1).  Returns the dict u,
        x, pi, lam, t of (nprob, nrhs, size) device tensors -- those of kkt_buffers(nrhs), overwritten by the next call.
        Neither the packed data nor the solver's iterate is written; ws only with refactor.  Asynchronous."""
        p0, count = self._range(p0, count)
        o = self.kkt_buffers(nrhs)
        ins = [self._tensor(sets.get(key), (self.nprob, nrhs, self.sizes[key]), f"set {key}",
                            optional=key == "z" or self.sizes[key] == 0) for key in SET_KEYS]
        base = (self.lam.data_ptr(), self.t.data_ptr()) if refactor else (None, None)
        check(lib().hpmpc_mi355x_soft_kkt_ocp_batch(
            self.plan, self.nprob, p0, count, nrhs, self.BAbt.data_ptr(), self.RSQrq.data_ptr(), self.Zp.data_ptr(),
            self.zp.data_ptr(), *base, *ins, o["u"].data_ptr(), o["x"].data_ptr(), o["pi"].data_ptr(),
            o["lam"].data_ptr(), o["t"].data_ptr(), self.ws.data_ptr(), o["work"].data_ptr(), o["scratch"].data_ptr(),
            1 if refactor else 0, self._stream()), "hpmpc_mi355x_soft_kkt_ocp_batch")
        s = self.sizes
        n = dict(u=s["u"], x=s["x"], pi=s["pi_out"], lam=s["lam_out"], t=s["lam_out"])
        return {key: o[key][..., :n[key]] for key in n}

    def resolve(self, data, refactor=True) -> dict:
        """One set per problem: the re-solve for the b, q, r, lb, ub (and z) of ``data`` ({key: (nprob, size) device
        tensor}; its matrices are not read).  Nothing is packed into the solver's own arrays and its iterate is left
        alone, so a finish() afterwards still returns the solve's outputs.  Returns u, x, pi, lam, t as (nprob, size)
        tensors: the keys of finish() without kk, status and norms."""
        sets = {key: data[key].reshape(self.nprob, 1, -1) for key in SET_KEYS if data.get(key) is not None}
        return {key: v[:, 0] for key, v in self.kkt_sets(sets, 1, refactor=refactor).items()}

    def results(self, out=None) -> list:
        """finish()'s tensors on the host, one interface-form dict per problem (synchronises)."""
        out = self.finish() if out is None else out
        self.torch.cuda.synchronize(self.dev)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        per = unflatten_soft_outputs(host, self.N, self.nx, self.nu, self.nb, self.ns)
        k_max = getattr(self, "_stat_kmax", self.k_max)
        stat = self.stat.cpu().numpy().reshape(-1)[:self.nprob * 5 * max(k_max, 1)].reshape(self.nprob, -1)
        for p, r in enumerate(per):
            r.update(kk=int(host["kk"][p]), status=int(host["status"][p]),
                     stat=stat[p, :5 * max(int(host["kk"][p]), 0)].copy())
            if "inf_norm_res" in host:
                r["inf_norm_res"] = host["inf_norm_res"][p].copy()
        return per

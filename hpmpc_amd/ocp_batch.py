"""Batched OCP front end: dense problem data in HBM -> pack -> IPM -> the c_interface.h wrappers' outputs.

The one-problem wrappers fortran_order_d_ip_ocp_hard_tv / c_order_d_ip_ocp_hard_tv take dense stage matrices from
the host; ``OcpBatchSolver`` is their top layer for ``nprob`` problems that share stage sizes and box indices and
whose dense data are torch tensors on the device (hpmpc_mi355x_ocp_* in include/hpmpc_mi355x.h, hk_ocp.hip).  torch is
plumbing here (allocation, streams); packing, the solve and the outputs are HIP kernels.

Dense arrays, per problem: the stage blocks concatenated in stage order,

    A_k (nx[k+1] x nx[k]), B_k (nx[k+1] x nu[k]), b_k    k < N       Q_k (nx x nx), q_k                k <= N
    S_k (nu x nx), R_k (nu x nu), r_k                     k < N       lb_k, ub_k (nb), C_k (ng x nx), lg_k, ug_k  k <= N
    D_k (ng x nu)                                         k < N

each matrix block row-major (order "C", the c_order_ convention) or column-major (order "F", fortran_order_).  The
outputs u, x, pi have the shapes of r, q, b; lam and t are compact, [lb nb | ub nb | lg ng | ug ng] per stage.
The host-side helpers below (numpy only, no library load) compute that layout and flatten / unflatten problems in
the interface form of oracle/iface_oracle.py random_iface_problem.
"""
from __future__ import annotations

import ctypes as C

import numpy as np

from .bindings import check, lib, plan_args
from .device import DeviceSolver

KEYS = ("A", "B", "b", "Q", "S", "R", "q", "r", "lb", "ub", "C", "D", "lg", "ug")  # HkOcpArray / hpmpc_mi355x_ocp_data
OUT_KEYS = ("u", "x", "pi", "lam", "t")
NSIZES, NOFFSETS = 29, 18  # HPMPC_MI355X_OCP_NSIZES / _NOFFSETS
# indices into hpmpc_mi355x_ocp_sizes beyond the 14 dense arrays
SZ = dict(BAbt=14, RSQrq=15, DCt=16, d=17, ux=18, pi=19, lam=20, ws=21, res=22, u=23, x=24, pi_out=25, lam_out=26,
          inf_norm_res=27, N=28)


def _shape(key, N, nx, nu, nb, ng, k):
    """Shape of stage k's block of a dense or output array (a stage without the block has a zero dimension)."""
    nuk = int(nu[k]) if k < N else 0
    nxk, nbk, ngk = int(nx[k]), int(nb[k]), int(ng[k])
    nx1 = int(nx[k + 1]) if k < N else 0
    return {"A": (nx1, nxk), "B": (nx1, nuk), "b": (nx1,), "Q": (nxk, nxk), "S": (nuk, nxk), "R": (nuk, nuk),
            "q": (nxk,), "r": (nuk,), "lb": (nbk,), "ub": (nbk,), "C": (ngk, nxk), "D": (ngk, nuk), "lg": (ngk,),
            "ug": (ngk,), "u": (nuk,), "x": (nxk,), "pi": (nx1,), "lam": (2 * nbk + 2 * ngk,),
            "t": (2 * nbk + 2 * ngk,)}[key]


def ocp_dense_layout(N, nx, nu, nb, ng) -> dict:
    """Doubles per problem (``sizes[key]``) and per-stage offsets (``offsets[key]``, N+1 entries) of every dense
    array and of the outputs u, x, pi, lam, t: the formulas of hpmpc_mi355x_ocp_sizes / _offsets."""
    sizes, offsets = {}, {}
    for key in KEYS + OUT_KEYS:
        off, o = np.zeros(N + 1, dtype=np.int64), 0
        for k in range(N + 1):
            off[k] = o
            o += int(np.prod(_shape(key, N, nx, nu, nb, ng, k)))
        sizes[key], offsets[key] = o, off
    return dict(sizes=sizes, offsets=offsets)


def _sizes_of(P):
    return P["N"], P["nx"], P["nu"], P["nb"], P["ng"]


def flatten_problems(problems, order="C", keys=KEYS) -> dict:
    """Interface-form problems (same sizes) -> {key: (nprob, size) float64}: each problem's stage blocks flattened
    in ``order`` ("C" row-major, "F" column-major) and concatenated in stage order.  Lists shorter than N+1 (A, B, b
    with N blocks) are taken as they are."""
    N, nx, nu, nb, ng = _sizes_of(problems[0])
    lay = ocp_dense_layout(N, nx, nu, nb, ng)
    out = {}
    for key in keys:
        arr = np.zeros((len(problems), lay["sizes"][key]))
        for p, P in enumerate(problems):
            if _sizes_of(P) != (N, nx, nu, nb, ng):
                raise ValueError("the problems of a batch share their stage sizes")
            for k, M in enumerate(P[key]):
                M = np.asarray(M, dtype=np.float64)
                shp = _shape(key, N, nx, nu, nb, ng, k)
                if M.size != int(np.prod(shp)):
                    raise ValueError(f"{key}[{k}] has {M.size} entries, expected shape {shp}")
                o = lay["offsets"][key][k]
                arr[p, o:o + M.size] = M.reshape(shp).flatten(order)
        out[key] = arr
    return out


def unflatten_problems(flat, N, nx, nu, nb, ng, order="C", keys=None) -> list:
    """Inverse of flatten_problems, for dense arrays and for the outputs u, x, pi, lam, t alike: {key: (nprob, size)}
    -> one dict per problem of per-stage blocks.  A, B, b, u, pi get N blocks, the others N+1 (the interface form:
    stage N's S, R, r, D blocks are empty)."""
    keys = [k for k in KEYS + OUT_KEYS if k in flat] if keys is None else keys
    lay = ocp_dense_layout(N, nx, nu, nb, ng)
    nprob = len(np.asarray(flat[keys[0]]))
    out = []
    for p in range(nprob):
        P = {}
        for key in keys:
            row = np.asarray(flat[key])[p]
            nblk = N if key in ("A", "B", "b", "u", "pi") else N + 1
            blocks = []
            for k in range(nblk):
                shp = _shape(key, N, nx, nu, nb, ng, k)
                o = lay["offsets"][key][k]
                blocks.append(row[o:o + int(np.prod(shp))].reshape(shp, order=order).copy())
            P[key] = blocks
        out.append(P)
    return out


def flatten_sets(sets, nsets, keys, order="C") -> dict:
    """flatten_problems for ``nsets`` sets per problem: ``sets[p][r]`` is set r of problem p in the interface form ->
    {key: (nprob, nsets, size) float64}."""
    flat = flatten_problems([S for per in sets for S in per[:nsets]], order, keys)
    return {key: v.reshape(len(sets), nsets, -1) for key, v in flat.items()}


def kkt_set_arrays(problems):
    """The per-set arrays of the batched KKT re-solve from interface-form problems (one set each, same sizes):
    b (n, N+1, 16) with b_k in state order, q (n, N+1, 16) in variable order [r_k | q_k], d (n, N+1, 32) as
    [lb pnb | ub pnb | lg png | ug png], padding zero -- the vectors hpmpc_amd.cabi.bq_from_qp extracts from the
    packed problem and the d of oracle/iface_oracle.py to_qp, element for element.  For ``nrhs`` sets per problem
    order the sets problem-major and reshape to (nprob, nrhs, N+1, .)."""
    N, nx, nu, nb, ng = _sizes_of(problems[0])
    n = len(problems)
    b, q, d = np.zeros((n, N + 1, 16)), np.zeros((n, N + 1, 16)), np.zeros((n, N + 1, 32))
    for p, P in enumerate(problems):
        if _sizes_of(P) != (N, nx, nu, nb, ng):
            raise ValueError("the problems of a batch share their stage sizes")
        for k in range(N + 1):
            nuk = int(nu[k]) if k < N else 0
            nxk, nbk, ngk = int(nx[k]), int(nb[k]), int(ng[k])
            pnb, png = (nbk + 3) // 4 * 4, (ngk + 3) // 4 * 4
            if k < N:
                b[p, k, :int(nx[k + 1])] = P["b"][k]
                q[p, k, :nuk] = P["r"][k]
            q[p, k, nuk:nuk + nxk] = P["q"][k]
            d[p, k, :nbk] = P["lb"][k]
            d[p, k, pnb:pnb + nbk] = P["ub"][k]
            d[p, k, 2 * pnb:2 * pnb + ngk] = P["lg"][k]
            d[p, k, 2 * pnb + png:2 * pnb + png + ngk] = P["ug"][k]
    return b, q, d


VEC_KEYS = ("b", "q", "r", "lb", "ub", "lg", "ug")  # the dense arrays a tangent direction may have
MAT_KEYS = ("A", "B", "Q", "S", "R", "C", "D")  # the others: matrix_gradients / adjoint_data, matrix_directions / tangent_data


def tangent_set_arrays(problem_deltas):
    """The direction twin of kkt_set_arrays: interface-form DELTAS (dicts with N, nx, nu, nb, ng and any of b, q, r,
    lb, ub, lg, ug as per-stage lists; a missing key is a zero direction) -> db (n, N+1, 16) in state order, dq
    (n, N+1, 16) in variable order [dr_k | dq_k], dd (n, N+1, 32) as [dlb pnb | dub pnb | dlg png | dug png], padding
    zero -- the arrays of hpmpc_mi355x_kkt_tangent_batch.  The placement is kkt_set_arrays' own, so for deltas that
    are exactly representable kkt_set_arrays(P + delta) - kkt_set_arrays(P) equals the result bit for bit."""
    N, nx, nu, nb, ng = _sizes_of(problem_deltas[0])
    full = []
    for D in problem_deltas:
        Z = dict(D)
        for key in VEC_KEYS:
            if Z.get(key) is None:
                nblk = N if key in ("b", "r") else N + 1
                Z[key] = [np.zeros(_shape(key, N, nx, nu, nb, ng, k)) for k in range(nblk)]
        full.append(Z)
    return kkt_set_arrays(full)


def adjoint_set_arrays(problem_cotangents):
    """The cotangent twin of tangent_set_arrays: dense interface-form COTANGENTS (dicts with N, nx, nu, nb, ng and any
    of u, x, pi, lam, t as per-stage lists shaped like the outputs -- lam / t compact [lb nb | ub nb | lg ng | ug ng];
    a missing key is zero) -> gux (n, N+1, 16) in variable order [gu_k | gx_k], gpi (n, N+1, 16) in state order, glam,
    gt (n, N+1, 32) as [lb pnb | ub pnb | lg png | ug png], padding zero -- the arrays of
    hpmpc_mi355x_kkt_adjoint_batch.  The placement is the transpose of the dense outputs' (the gather a padded iterate
    goes through on its way to u, x, pi, lam, t, without the equality-box fix): sum(dense(it) * g) == sum(it *
    adjoint_set_arrays(g)) for every padded iterate it."""
    N, nx, nu, nb, ng = _sizes_of(problem_cotangents[0])
    n = len(problem_cotangents)
    gux, gpi = np.zeros((n, N + 1, 16)), np.zeros((n, N + 1, 16))
    glam, gt = np.zeros((n, N + 1, 32)), np.zeros((n, N + 1, 32))
    for p, G in enumerate(problem_cotangents):
        if _sizes_of(G) != (N, nx, nu, nb, ng):
            raise ValueError("the problems of a batch share their stage sizes")
        blk = lambda key, k: None if G.get(key) is None or k >= len(G[key]) else np.asarray(G[key][k], dtype=np.float64)
        for k in range(N + 1):
            nuk = int(nu[k]) if k < N else 0
            nxk, nbk, ngk = int(nx[k]), int(nb[k]), int(ng[k])
            pnb, png = (nbk + 3) // 4 * 4, (ngk + 3) // 4 * 4
            if k < N and blk("u", k) is not None:
                gux[p, k, :nuk] = blk("u", k)
            if blk("x", k) is not None:
                gux[p, k, nuk:nuk + nxk] = blk("x", k)
            if k < N and blk("pi", k) is not None:
                gpi[p, k, :int(nx[k + 1])] = blk("pi", k)
            for key, arr in (("lam", glam), ("t", gt)):
                v = blk(key, k)
                if v is None:
                    continue
                if v.shape != (2 * nbk + 2 * ngk,):
                    raise ValueError(f"{key}[{k}] has shape {v.shape}, expected {(2 * nbk + 2 * ngk,)}")
                arr[p, k, :nbk] = v[:nbk]
                arr[p, k, pnb:pnb + nbk] = v[nbk:2 * nbk]
                arr[p, k, 2 * pnb:2 * pnb + ngk] = v[2 * nbk:2 * nbk + ngk]
                arr[p, k, 2 * pnb + png:2 * pnb + png + ngk] = v[2 * nbk + ngk:]
    return gux, gpi, glam, gt


def x0_directions(A0, S0=None):
    """The nx0 parameter directions of an initial state x_0 that is folded into stage 0 (nx[0] = 0, b_0 = A_0 x_0 + b,
    r_0 = r + S_0 x_0): direction i is db_0 = A_0[:, i] and, with S0, dr_0 = S_0[:, i].  A0: (..., nx[1], nx0), S0:
    (..., nu[0], nx0), numpy arrays or torch tensors with any leading batch shape.  Returns the stage-0 blocks
    {"b": (..., nx0, nx[1]), "r": (..., nx0, nu[0])} (no "r" without S0); every other stage's direction is zero.
    OcpBatchSolver.feedback_gain embeds them into the (nprob, ndir, size) tensors of tangent()."""
    out = {"b": A0.swapaxes(-1, -2)}
    if S0 is not None:
        if S0.shape[-1] != A0.shape[-1]:
            raise ValueError("A0 and S0 have one column per component of x_0")
        out["r"] = S0.swapaxes(-1, -2)
    return out


class _OcpData(C.Structure):
    _fields_ = [("ptr", C.c_void_p * len(KEYS)), ("stride", C.c_longlong * len(KEYS))]


class _OcpGrads(C.Structure):
    _fields_ = [("ptr", C.c_void_p * len(KEYS)), ("stride", C.c_longlong * len(KEYS))]


ocp_lib = lib  # the hpmpc_mi355x_ocp_* calls are bound with every other one (hpmpc_amd.bindings)


def ocp_plan_create(N, nx, nu, nb, idxb, ng, order="C"):
    """(plan handle or None, error code, keep-alive objects) of hpmpc_mi355x_ocp_plan_create."""
    L = lib()
    nuv = list(nu) + [0] * (N + 1 - len(nu))
    (pnx, pnu, pnb, png), idxp, keep = plan_args(idxb, nx, nuv, nb, ng)
    plan = L.hpmpc_mi355x_ocp_plan_create(N, pnx, pnu, pnb, idxp, png, 1 if order == "C" else 0)
    return (plan or None), L.hpmpc_mi355x_last_error(), keep


class OcpBatchSolver(DeviceSolver):
    """``nprob`` OCPs with the given stage sizes: owns the lib4 arrays, the iterate, the workspaces and the outputs
    (torch tensors on ``device``).  pack() -> solve() -> finish(), then any number of resolve() -> finish() or
    kkt_sets() / tangent() / tangent_data() / adjoint() / adjoint_data() on the factor solve() left, all asynchronous on
    torch's current stream.
    There is no CPU fallback: without a GPU or the built library the constructor raises."""

    _destroy = "hpmpc_mi355x_ocp_plan_destroy"

    def __init__(self, N, nx, nu, nb, idxb, ng, nprob, order="C", device="cuda", k_max=50):
        if order not in ("C", "F"):
            raise ValueError("order is 'C' (row-major blocks) or 'F' (column-major blocks)")
        super().__init__(device)
        torch = self.torch
        self.N, self.nprob, self.k_max, self.order = int(N), int(nprob), int(k_max), order
        self.nx, self.nu = [int(v) for v in nx], [int(v) for v in nu][:N] + [0]
        self.nb, self.ng = [int(v) for v in nb], [int(v) for v in ng]
        L = lib()
        self.plan, err, self._keep = ocp_plan_create(N, self.nx, self.nu, self.nb, idxb, self.ng, order)
        if not self.plan:
            raise ValueError(f"unsupported problem sizes for the batched OCP front end (code {err})")
        sz = np.zeros(NSIZES, dtype=np.int64)
        L.hpmpc_mi355x_ocp_sizes(self.plan, sz.ctypes.data)
        self.sizes = {k: int(sz[i]) for i, k in enumerate(KEYS)}
        self.sizes.update({k: int(sz[i]) for k, i in SZ.items()})
        off = np.zeros((N + 1, NOFFSETS), dtype=np.int64)
        L.hpmpc_mi355x_ocp_offsets(self.plan, off.ctypes.data)
        self.offsets = {k: off[:, i].copy() for i, k in enumerate(KEYS)}
        self.offsets.update(lam_out=off[:, 14].copy(), BAbt=off[:, 15].copy(), RSQrq=off[:, 16].copy(),
                            DCt=off[:, 17].copy())
        P, s = self.nprob, self.sizes
        new = lambda n, dt=torch.float64: torch.zeros((P, max(n, 1)), dtype=dt, device=self.dev)
        self.BAbt, self.RSQrq, self.DCt, self.d = new(s["BAbt"]), new(s["RSQrq"]), new(s["DCt"]), new(s["d"])
        self.ux, self.pi, self.lam, self.t = new(s["ux"]), new(s["pi"]), new(s["lam"]), new(s["lam"])
        self.ws, self.res = new(s["ws"]), new(s["res"])
        self.u, self.x, self.pi_out = new(s["u"]), new(s["x"]), new(s["pi_out"])
        self.lam_out, self.t_out = new(s["lam_out"]), new(s["lam_out"])
        self.inf_norm_res = new(4)
        self.kk = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.ret = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.stat = new(5 * max(self.k_max, 1))

    def _vec(self, x, n, what):
        """(pointer, problem stride) of a float64 device tensor: (nprob, n) with unit inner stride (the rows may be
        apart), or (n,) shared by every problem (stride 0)."""
        if x.dim() == 2 and x.shape[0] == self.nprob:
            return self._tensor(x[0], (n,), what), x.stride(0)  # the first row's pointer is the tensor's
        return self._tensor(x, (n,), what), 0

    def _ocp_data(self, data, one):
        """hpmpc_mi355x_ocp_data of {key: tensor}: ``one(key, x, n)`` gives (pointer, stride) of a given array of
        sizes[key] = n, or raises; a missing (or None) one is null."""
        ds = _OcpData()
        for i, key in enumerate(KEYS):
            x = data.get(key)
            ds.ptr[i], ds.stride[i] = (None, 0) if x is None else one(key, x, self.sizes[key])
        return ds

    def data_struct(self, data):
        for key in KEYS:
            if self.sizes[key] and data.get(key) is None:
                raise ValueError(f"dense array {key} missing")
        return self._ocp_data(data, lambda key, x, n: self._vec(x, n, key))

    def _lib4(self, ptr=True):
        """The packed BAbt, RSQrq and DCt (None without general constraints), as pointers or as tensors."""
        arrays = self.BAbt, self.RSQrq, self.DCt if self.sizes["DCt"] else None
        return tuple(None if x is None else x.data_ptr() for x in arrays) if ptr else arrays

    def _out_sizes(self):
        s = self.sizes
        return dict(u=s["u"], x=s["x"], pi=s["pi_out"], lam=s["lam_out"], t=s["lam_out"])

    def _sized(self, o):
        """The tensors u, x, pi, lam, t of ``o``, allocated with at least one element, cut to their sizes."""
        return {key: o[key][..., :n] for key, n in self._out_sizes().items()}

    def pack(self, data, matrices=True, warm=None, p0=0, count=None):
        """Dense device tensors -> BAbt, RSQrq, DCt, d (hk_ocp_pack).  ``data``: {key: tensor (nprob, size), or
        (size,) for an array shared by every problem (stride 0)}.  matrices=False rewrites only b, q, r and the
        bounds.  warm: {"u": (nprob, sizes["u"]), "x": (nprob, sizes["x"])} packed into ux for warm_start=1."""
        p0, count = self._range(p0, count)
        ds = self.data_struct(data)
        u0 = x0 = ux = None
        if warm is not None:
            u0, su = self._vec(warm["u"], self.sizes["u"], "warm u")
            x0, sx = self._vec(warm["x"], self.sizes["x"], "warm x")
            if (su, sx) != (self.sizes["u"], self.sizes["x"]) and self.nprob > 1:
                raise ValueError("warm u / x: contiguous (nprob, size) tensors expected")
            ux = self.ux.data_ptr()
        check(lib().hpmpc_mi355x_ocp_pack_batch(
            self.plan, C.byref(ds), 1 if matrices else 0, self.nprob, p0, count, *self._lib4(), self.d.data_ptr(), u0,
            x0, ux, self._stream()), "hpmpc_mi355x_ocp_pack_batch")

    def solve(self, mu0=2.0, mu_tol=1e-10, alpha_min=1e-8, warm_start=0, p0=0, count=None):
        """d_ip2_res_mpc_hard_tv on the packed batch (mu0 > 0: one value for the batch)."""
        p0, count = self._range(p0, count)
        check(lib().hpmpc_mi355x_ocp_ipm_batch(
            self.plan, self.nprob, p0, count, *self._lib4(), self.d.data_ptr(), self.ux.data_ptr(), self.pi.data_ptr(),
            self.lam.data_ptr(), self.t.data_ptr(), self.ws.data_ptr(), self.k_max, mu0, mu_tol, alpha_min, warm_start, 1, self.kk.data_ptr(), self.ret.data_ptr(), self.stat.data_ptr(),
            self._stream()), "hpmpc_mi355x_ocp_ipm_batch")

    def kkt_buffers(self, nrhs: int = 1) -> dict:
        """The output and scratch tensors kkt_sets(nrhs=nrhs) writes (allocated on first use, then reused);
        resolve() uses the scratch of nrhs = 1."""
        from .batch import kkt_buffers

        return self._per_set("kkt", nrhs, lambda n: kkt_buffers(
            self.torch, self.dev, lib().hpmpc_mi355x_ocp_tile_plan(self.plan), self.N, self.nprob, n))

    def _dense_sets(self, kind, nsets, sizes):
        """The cached dict {key: zeros (nprob, nsets, max(size, 1))} over ``sizes`` = {key: size}."""
        return self._per_set(kind, nsets, lambda n: {key: self.torch.zeros(
            (self.nprob, n, max(size, 1)), dtype=self.torch.float64, device=self.dev) for key, size in sizes.items()})

    def resolve(self, data, p0=0, count=None):
        """The batched c_order_ / fortran_order_d_solve_kkt_new_rhs_ocp_hard_tv: re-solve the last Newton system of
        solve() for the b, q, r and bounds of ``data`` (dense tensors as for pack(); its matrices are not read).
        The vectors-only pack, then hpmpc_mi355x_ocp_kkt_batch into the solver's own iterate (ux, pi, lam, t);
        finish() then gives the wrapper's outputs (its kk / status are still solve()'s).  ws keeps the factor, so
        resolve() may be called again with other data.  Needs a solve() with at least one iteration."""
        p0, count = self._range(p0, count)
        self.pack(data, matrices=False, p0=p0, count=count)
        check(lib().hpmpc_mi355x_ocp_kkt_batch(
            self.plan, self.nprob, p0, count, *self._lib4(), self.d.data_ptr(), self.ux.data_ptr(), self.pi.data_ptr(),
            self.lam.data_ptr(), self.t.data_ptr(), self.ws.data_ptr(), self.kkt_buffers(1)["scratch"].data_ptr(), self._stream()), "hpmpc_mi355x_ocp_kkt_batch")

    def kkt_sets(self, b, q, d, nrhs=1, p0=0, count=None, compute_mult=1, dense=False):
        """hpmpc_mi355x_kkt_new_rhs_batch with the tile plan on the packed arrays: ``nrhs`` right-hand-side sets per
        problem against the factor of solve().  b, q: (nprob, nrhs, N+1, 16) device tensors or None (the rows
        packed into BAbt / RSQrq); d: (nprob, nrhs, N+1, 32) (kkt_set_arrays builds all three).  Returns ux, pi,
        lam, t with a leading (nprob, nrhs) shape in the padded layouts of the iterate -- the tensors of
        kkt_buffers(nrhs).  Neither ws nor the solver's iterate is written.
        dense=True: the sets are then unpacked on the device (hpmpc_mi355x_ocp_unpack_sets, the equality-box fix
        from each set's own d) and the call returns the dict u, x, pi, lam, t of (nprob, nrhs, size) tensors --
        those of set_buffers(nrhs); per set what resolve() -> finish() gives on that set's data, without the
        residual norms."""
        from .batch import kkt_sets_call

        p0, count = self._range(p0, count)
        out = self.kkt_buffers(nrhs)
        check(kkt_sets_call(self.torch, lib().hpmpc_mi355x_ocp_tile_plan(self.plan), None, self.N, self.nprob, p0,
                            count, nrhs, *self._lib4(ptr=False), b, q, d, out,
                            self.ws, compute_mult, self._stream()), "hpmpc_mi355x_kkt_new_rhs_batch")
        if not dense:
            return out["ux"], out["pi"], out["lam"], out["t"]
        o = self.set_buffers(nrhs)
        check(lib().hpmpc_mi355x_ocp_unpack_sets(
            self.plan, self.nprob, p0, count, nrhs, d.data_ptr(), out["ux"].data_ptr(), out["pi"].data_ptr(),
            out["lam"].data_ptr(), out["t"].data_ptr(), o["u"].data_ptr(), o["x"].data_ptr(), o["pi"].data_ptr(),
            o["lam"].data_ptr(), o["t"].data_ptr(), self._stream()), "hpmpc_mi355x_ocp_unpack_sets")
        return self._sized(o)

    def set_buffers(self, nsets: int = 1) -> dict:
        """The dense per-set tensors u, x, pi, lam, t of shape (nprob, nsets, max(size, 1)) that tangent(ndir=nsets)
        and kkt_sets(nrhs=nsets, dense=True) write (allocated on first use, then reused and overwritten)."""
        return self._dense_sets("sets", nsets, self._out_sizes())

    def tangent(self, dirs, ndir, p0=0, count=None, compute_mult=1):
        """Forward sensitivities of the re-solved plan (hpmpc_mi355x_ocp_tangent_batch): the directional derivative
        of what resolve() computes with respect to its b, q, r and bounds, ``ndir`` directions per problem in one
        launch on the factor of solve().  ``dirs``: {key: contiguous float64 device tensor (nprob, ndir,
        sizes[key])} for any of b, q, r, lb, ub, lg, ug; a missing (or None) key is a zero direction.  A matrix key
        is passed on and refused by the library: directions in A, B, Q, S, R, C, D are tangent_data()'s.  Returns the dict
        u, x, pi, lam, t of (nprob, ndir, size) tensors (du, dx, dpi, compact dlam, dt) -- those of
        set_buffers(ndir).  The equality-box fix of finish() is not applied to tangents.  compute_mult=0: pi comes
        back as zeros.  Neither ws nor the solver's data or iterate is written."""
        p0, count = self._range(p0, count)
        # a matrix key's shape is not looked at: the library refuses the key itself
        ds = self._ocp_data(dirs, lambda key, x, n: (self._tensor(
            x, (self.nprob, ndir, n) if key in VEC_KEYS else x.shape, f"direction {key}"), n))
        o = self.set_buffers(ndir)
        check(lib().hpmpc_mi355x_ocp_tangent_batch(
            self.plan, C.byref(ds), self.nprob, p0, count, ndir, *self._lib4(), o["u"].data_ptr(), o["x"].data_ptr(),
            o["pi"].data_ptr(), o["lam"].data_ptr(), o["t"].data_ptr(), self.ws.data_ptr(),
            self.kkt_buffers(ndir)["scratch"].data_ptr(), compute_mult, self._stream()),
            "hpmpc_mi355x_ocp_tangent_batch")
        return self._sized(o)

    def tangent_sets(self, db, dq, dd, ndir=1, p0=0, count=None, compute_mult=1):
        """The padded core of tangent() (hpmpc_mi355x_kkt_tangent_batch with the tile plan on the packed arrays): db,
        dq (nprob, ndir, N+1, 16), dd (nprob, ndir, N+1, 32) device tensors (tangent_set_arrays builds them) or None
        for a zero direction.  Returns dux, dpi, dlam, dt with a leading (nprob, ndir) shape in the padded layouts of
        the iterate -- the ux, pi, lam, t tensors of kkt_buffers(ndir), which kkt_sets(nrhs=ndir) also writes."""
        from .batch import kkt_tangent_call

        p0, count = self._range(p0, count)
        out = self.kkt_buffers(ndir)
        check(kkt_tangent_call(self.torch, lib().hpmpc_mi355x_ocp_tile_plan(self.plan), None, self.N, self.nprob, p0,
                               count, ndir, *self._lib4(ptr=False), db, dq, dd,
                               out, self.ws, compute_mult, self._stream()), "hpmpc_mi355x_kkt_tangent_batch")
        return out["ux"], out["pi"], out["lam"], out["t"]

    def feedback_gain(self, A0, S0=None, p0=0, count=None):
        """d u_0 / d x_0, (nprob, nu[0], nx0), of a batch whose x_0 is folded into stage 0 (nx[0] = 0, b_0 = A_0 x_0 +
        b, r_0 = r + S_0 x_0): one tangent() with the nx0 directions of x0_directions(A0, S0).  A0: (nprob, nx[1],
        nx0) or (nx[1], nx0) for every problem, S0 likewise (nu[0], nx0) or None; numpy arrays or device tensors."""
        torch = self.torch
        if self.nx[0] != 0:
            raise ValueError("feedback_gain: x_0 is folded into stage 0 (nx[0] = 0)")
        dev = lambda M: None if M is None else torch.as_tensor(M, dtype=torch.float64).to(self.dev)
        blocks = x0_directions(dev(A0), dev(S0))
        nx0 = blocks["b"].shape[-2]
        dirs = {}
        for key, width in (("b", self.nx[1]), ("r", self.nu[0])):
            if key not in blocks:
                continue
            blk = blocks[key]
            if tuple(blk.shape[-2:]) != (nx0, width):
                raise ValueError(f"feedback_gain: the stage-0 block of {key} has {width} rows")
            full = torch.zeros((self.nprob, nx0, self.sizes[key]), dtype=torch.float64, device=self.dev)
            full[:, :, :width] = blk  # stage 0's block starts every problem's array; a 2-D block is shared
            dirs[key] = full
        du = self.tangent(dirs, nx0, p0=p0, count=count)["u"]
        return du[:, :, :self.nu[0]].transpose(1, 2)

    def grad_buffers(self, nadj: int = 1) -> dict:
        """The dense per-set gradient tensors b, q, r, lb, ub, lg, ug of shape (nprob, nadj, max(size, 1)) that
        adjoint(nadj=nadj) writes (allocated on first use, then reused and overwritten)."""
        return self._dense_sets("grads", nadj, {key: self.sizes[key] for key in VEC_KEYS})

    def _cot_ptrs(self, cot, nadj):
        """The pointers gu, gx, gpi, glam, gt of the dense cotangents ``cot`` (None: zero), after checking them."""
        ptrs = [self._tensor(cot.get(key), (self.nprob, nadj, n), f"cotangent {key}", optional=True)
                for key, n in self._out_sizes().items()]
        if any(key not in OUT_KEYS for key in cot):
            raise ValueError(f"cotangents are keyed by {OUT_KEYS}")
        return ptrs

    def adjoint(self, cot, nadj, p0=0, count=None, want=VEC_KEYS):
        """Reverse sensitivities of the re-solved plan (hpmpc_mi355x_ocp_adjoint_batch), the transpose of tangent():
        for ``nadj`` cotangent sets per problem -- each the gradient of a scalar loss with respect to what resolve()
        computes -- that loss's gradient with respect to b, q, r and the bounds, one Riccati solve per set on the
        factor of solve().  ``cot``: {key: contiguous float64 device tensor (nprob, nadj, size)} for any of u, x, pi,
        lam, t (the sizes of the outputs; lam / t compact); a missing (or None) key is zero.  Returns {key: (nprob,
        nadj, sizes[key])} over ``want`` (default all of b, q, r, lb, ub, lg, ug) -- tensors of grad_buffers(nadj);
        a key left out of ``want`` is not written, and without "b" the multiplier half of the solve is skipped.
        Neither ws nor the solver's data or iterate is written."""
        p0, count = self._range(p0, count)
        if not want or any(key not in VEC_KEYS for key in want):
            raise ValueError(f"want: a non-empty subset of {VEC_KEYS} expected")
        s = self.sizes
        ptrs = self._cot_ptrs(cot, nadj)
        g = self.grad_buffers(nadj)
        check(lib().hpmpc_mi355x_ocp_adjoint_batch(
            self.plan, self.nprob, p0, count, nadj, *self._lib4(), *ptrs,
            *(g[key].data_ptr() if key in want else None for key in VEC_KEYS), self.ws.data_ptr(),
            self.kkt_buffers(nadj)["scratch"].data_ptr(), self._stream()), "hpmpc_mi355x_ocp_adjoint_batch")
        return {key: g[key][..., :s[key]] for key in VEC_KEYS if key in want}

    def adjoint_sets(self, gux, gpi, glam, gt, nadj=1, p0=0, count=None, want_b=True):
        """The padded core of adjoint() (hpmpc_mi355x_kkt_adjoint_batch with the tile plan on the packed arrays): gux,
        gpi (nprob, nadj, N+1, 16), glam, gt (nprob, nadj, N+1, 32) device tensors (adjoint_set_arrays builds them) or
        None for zero.  Returns (bbar, qbar, dbar) with a leading (nprob, nadj) shape in the padded layouts of b, q and
        d -- the pi, ux, lam tensors of kkt_buffers(nadj), which kkt_sets / tangent_sets of that set count also write.
        want_b=False: the multiplier half is skipped, bbar is None and the pi buffer is not written."""
        from .batch import kkt_adjoint_call

        p0, count = self._range(p0, count)
        out = self.kkt_buffers(nadj)
        check(kkt_adjoint_call(self.torch, lib().hpmpc_mi355x_ocp_tile_plan(self.plan), None, self.N, self.nprob, p0,
                               count, nadj, *self._lib4(ptr=False), gux, gpi, glam, gt, out, self.ws, want_b,
                               self._stream()), "hpmpc_mi355x_kkt_adjoint_batch")
        return (out["pi"] if want_b else None), out["ux"], out["lam"]

    def matrix_grad_buffers(self, nadj: int = 1) -> dict:
        """The dense per-set gradient tensors A, B, Q, S, R, C, D of shape (nprob, nadj, max(size, 1)) that
        matrix_gradients(nadj=nadj) and adjoint_data(nadj=nadj) write (allocated on first use, then reused and
        overwritten)."""
        return self._dense_sets("matrix_grads", nadj, {key: self.sizes[key] for key in MAT_KEYS})

    def _grads_struct(self, bufs, want):
        """hpmpc_mi355x_ocp_grads over the tensors ``bufs`` (nprob, nadj, >= size): the keys of ``want``, else null."""
        gs = _OcpGrads()
        for i, key in enumerate(KEYS):
            gs.ptr[i], gs.stride[i] = (bufs[key].data_ptr(), bufs[key].shape[-1]) if key in want else (None, 0)
        return gs

    def _base_ptrs(self, base):
        """Pointers of the padded base iterate ux, pi, lam: the solver's own (the raw iterate solve() or resolve() left,
        without finish()'s equality-box fix), or ``base`` = dict(ux=, pi=, lam=) of (nprob, sizes[key]) tensors."""
        if base is None:
            return self.ux.data_ptr(), self.pi.data_ptr(), self.lam.data_ptr()
        return tuple(self._tensor(base[key], (self.nprob, self.sizes[key]), f"base {key}")
                     for key in ("ux", "pi", "lam"))

    def matrix_gradients(self, bbar, qbar, dbar, nadj, want=MAT_KEYS, base=None, p0=0, count=None):
        """Gradients with respect to the matrices from an adjoint solution (hpmpc_mi355x_ocp_matrix_grads_batch, one
        launch): bbar, qbar (nprob, nadj, N+1, 16), dbar (nprob, nadj, N+1, 32) as adjoint_sets returns them (bbar may
        be None without "A" and "B"), and the base iterate (``base``, default the solver's own ux, pi, lam).  Per stage
        gA = bbar x' + pi qxbar', gB = bbar u' + pi rbar', gQ = (qxbar x' + x qxbar') / 2, gR = (rbar u' + u rbar') / 2,
        gS = rbar x' + u qxbar', gC = w qxbar' - s x', gD = w rbar' - s u' with w = lam_ug - lam_lg, s = dbar_lg +
        dbar_ug; gQ / gR are the gradients for symmetric perturbations.  This is the transpose of the linearised KKT
        system on the persisted factor, not the derivative of a fully converged solve (include/hpmpc_mi355x.h).
        Returns {key: (nprob, nadj, sizes[key])} over ``want`` -- tensors of matrix_grad_buffers(nadj); blocks in the
        solver's order ("C" row-major / "F" column-major).  No input is written."""
        p0, count = self._range(p0, count)
        if not want or any(key not in MAT_KEYS for key in want):
            raise ValueError(f"want: a non-empty subset of {MAT_KEYS} expected")
        bars = [self._tensor(x, (self.nprob, nadj, self.N + 1, w), name, optional)
                for name, x, w, optional in (("bbar", bbar, 16, "A" not in want and "B" not in want),
                                             ("qbar", qbar, 16, False), ("dbar", dbar, 32, False))]
        g = self.matrix_grad_buffers(nadj)
        gs = self._grads_struct(g, want)
        check(lib().hpmpc_mi355x_ocp_matrix_grads_batch(
            self.plan, self.nprob, p0, count, nadj, *self._base_ptrs(base), *bars, C.byref(gs), self._stream()),
            "hpmpc_mi355x_ocp_matrix_grads_batch")
        return {key: g[key][..., :self.sizes[key]] for key in MAT_KEYS if key in want}

    def adjoint_data(self, cot, nadj, want=KEYS, base=None, p0=0, count=None):
        """Gradients with respect to any of the fourteen data arrays (hpmpc_mi355x_ocp_adjoint_data_batch): adjoint()'s
        launch, then matrix_gradients()'s on the adjoint solution in the scratch, on one stream with nothing in
        between.  ``cot`` as for adjoint(); ``base`` as for matrix_gradients().  Returns {key: (nprob, nadj,
        sizes[key])} over ``want`` -- the vector keys are tensors of grad_buffers(nadj) and bit for bit adjoint()'s, the
        matrix keys tensors of matrix_grad_buffers(nadj) and bit for bit adjoint_sets() -> matrix_gradients()'s.
        Wanting "A" or "B" runs the multiplier half of the solve even without "b"."""
        p0, count = self._range(p0, count)
        if not want or any(key not in KEYS for key in want):
            raise ValueError(f"want: a non-empty subset of {KEYS} expected")
        ptrs = self._cot_ptrs(cot, nadj)
        g = dict(self.grad_buffers(nadj))
        if any(key in MAT_KEYS for key in want):
            g.update(self.matrix_grad_buffers(nadj))
        gs = self._grads_struct(g, want)
        check(lib().hpmpc_mi355x_ocp_adjoint_data_batch(
            self.plan, self.nprob, p0, count, nadj, *self._lib4(), *self._base_ptrs(base), *ptrs, C.byref(gs),
            self.ws.data_ptr(), self.kkt_buffers(nadj)["scratch"].data_ptr(), self._stream()),
            "hpmpc_mi355x_ocp_adjoint_data_batch")
        return {key: g[key][..., :self.sizes[key]] for key in KEYS if key in want}

    def direction_buffers(self, ndir: int = 1) -> dict:
        """The padded per-set seed rows db, dq (nprob, ndir, N+1, 16) and dd (nprob, ndir, N+1, 32) that
        matrix_directions(ndir=ndir) writes (allocated on first use, then reused and overwritten).  They are not the
        kkt_buffers tensors, so tangent_sets() may read them while it writes its own."""
        zeros = lambda n, w: self.torch.zeros((self.nprob, n, self.N + 1, w), dtype=self.torch.float64, device=self.dev)
        return self._per_set("dirs", ndir, lambda n: dict(db=zeros(n, 16), dq=zeros(n, 16), dd=zeros(n, 32)))

    def _dirs_struct(self, dirs, ndir):
        """hpmpc_mi355x_ocp_data of the direction tensors {key: (nprob, ndir, sizes[key])} over any of the fourteen
        arrays (strides between sets); a missing (or None) key is null."""
        if any(key not in KEYS for key in dirs):
            raise ValueError(f"directions are keyed by {KEYS}")
        return self._ocp_data(dirs, lambda key, x, n: (self._tensor(x, (self.nprob, ndir, n), f"direction {key}"), n))

    def matrix_directions(self, dirs, ndir, base=None, p0=0, count=None):
        """The seed rows of directions in any of the fourteen data arrays (hpmpc_mi355x_ocp_matrix_dirs_batch, one
        launch): per stage db = db + dA x + dB u, dr = dr + sym(dR) u + dS x + dB' pi + dD' w, dq = dq + sym(dQ) x +
        dS' u + dA' pi + dC' w, dd_lg / dd_ug = dlg / dug - (dC x + dD u), with w = lam_ug - lam_lg and sym(M) =
        (M + M') / 2, at the base iterate (``base``, default the solver's own ux, pi, lam; as for matrix_gradients).
        ``dirs``: {key: contiguous float64 device tensor (nprob, ndir, sizes[key])}, blocks in the solver's order; a
        missing (or None) vector key is a zero direction, a missing matrix key contributes nothing.  Returns (db, dq,
        dd), the tensors of direction_buffers(ndir), in the layouts tangent_sets() takes.  No input is written."""
        p0, count = self._range(p0, count)
        ds = self._dirs_struct(dirs, ndir)
        o = self.direction_buffers(ndir)
        check(lib().hpmpc_mi355x_ocp_matrix_dirs_batch(
            self.plan, C.byref(ds), self.nprob, p0, count, ndir, *self._base_ptrs(base), o["db"].data_ptr(),
            o["dq"].data_ptr(), o["dd"].data_ptr(), self._stream()), "hpmpc_mi355x_ocp_matrix_dirs_batch")
        return o["db"], o["dq"], o["dd"]

    def tangent_data(self, dirs, ndir, base=None, p0=0, count=None, compute_mult=1):
        """Forward sensitivities with respect to any of the fourteen data arrays (hpmpc_mi355x_ocp_tangent_data_batch):
        matrix_directions()'s launch into the sets' scratch, then tangent()'s solve on those seed rows, on one stream
        with nothing in between -- one Riccati solve per direction set gives the derivative of the whole plan.  ``dirs``
        and ``base`` as for matrix_directions().  Returns the dict u, x, pi, lam, t of (nprob, ndir, size) tensors --
        those of set_buffers(ndir); without matrix keys bit for bit tangent()'s.  This is the linearised KKT system on
        the persisted factor -- the forward twin of adjoint_data(): sum(g * tangent_data(d)) == sum(adjoint_data(g) * d)
        up to rounding, Q and R acting through their symmetric parts -- not the derivative of a fully converged solve
        (include/hpmpc_mi355x.h).  Neither ws nor the solver's data or iterate is written."""
        p0, count = self._range(p0, count)
        ds = self._dirs_struct(dirs, ndir)
        o = self.set_buffers(ndir)
        check(lib().hpmpc_mi355x_ocp_tangent_data_batch(
            self.plan, C.byref(ds), self.nprob, p0, count, ndir, *self._lib4(), *self._base_ptrs(base),
            o["u"].data_ptr(), o["x"].data_ptr(), o["pi"].data_ptr(), o["lam"].data_ptr(), o["t"].data_ptr(),
            self.ws.data_ptr(), self.kkt_buffers(ndir)["scratch"].data_ptr(), compute_mult, self._stream()),
            "hpmpc_mi355x_ocp_tangent_data_batch")
        return self._sized(o)

    def x0_gradient(self, A0, S0, grads):
        """The chain rule of x0_directions: the gradient with respect to an x_0 folded into stage 0 (b_0 = A_0 x_0 + b,
        r_0 = r + S_0 x_0), A_0' gb_0 + S_0' gr_0, from the ``grads`` adjoint() returned ("b", and "r" with S0).
        A0: (nprob, nx[1], nx0) or (nx[1], nx0), S0 likewise (nu[0], nx0) or None.  Returns (nprob, nadj, nx0)."""
        torch = self.torch
        if self.nx[0] != 0:
            raise ValueError("x0_gradient: x_0 is folded into stage 0 (nx[0] = 0)")
        dev = lambda M: torch.as_tensor(M, dtype=torch.float64).to(self.dev)
        # a 2-D block is shared by every problem
        mul = lambda M, g: torch.einsum("ji,prj->pri" if dev(M).dim() == 2 else "pji,prj->pri", dev(M), g)
        A0 = dev(A0)
        if A0.shape[-2] != self.nx[1]:
            raise ValueError(f"x0_gradient: A0 has {self.nx[1]} rows")
        out = mul(A0, grads["b"][:, :, :self.nx[1]])  # stage 0's block starts every problem's array
        if S0 is not None:
            if tuple(dev(S0).shape[-2:]) != (self.nu[0], A0.shape[-1]):
                raise ValueError("x0_gradient: A0 and S0 have one column per component of x_0")
            out = out + mul(S0, grads["r"][:, :, :self.nu[0]])
        return out

    def feedback_gain_adjoint(self, A0, S0=None, p0=0, count=None):
        """feedback_gain by reverse mode: d u_0 / d x_0, (nprob, nu[0], nx0), from nu[0] adjoint sets instead of nx0
        tangent sets -- set i has the cotangent e_i on u_0, and row i of the gain is its x0_gradient."""
        torch = self.torch
        if self.nx[0] != 0:
            raise ValueError("feedback_gain_adjoint: x_0 is folded into stage 0 (nx[0] = 0)")
        nu0 = self.nu[0]
        gu = torch.zeros((self.nprob, nu0, self.sizes["u"]), dtype=torch.float64, device=self.dev)
        idx = torch.arange(nu0, device=self.dev)
        gu[:, idx, idx] = 1.0  # stage 0's block starts every problem's u
        grads = self.adjoint({"u": gu}, nu0, p0=p0, count=count, want=("b",) if S0 is None else ("b", "r"))
        return self.x0_gradient(A0, S0, grads)

    def finish(self, p0=0, count=None) -> dict:
        """The wrappers' outputs as device tensors (nprob, size): u, x (equality-box fix applied), pi, compact lam
        and t, inf_norm_res (nprob, 4), kk and status per problem.  Asynchronous: synchronise before reading."""
        p0, count = self._range(p0, count)
        check(lib().hpmpc_mi355x_ocp_finish_batch(
            self.plan, self.nprob, p0, count, *self._lib4(), self.d.data_ptr(), self.ux.data_ptr(), self.pi.data_ptr(),
            self.lam.data_ptr(), self.t.data_ptr(), self.res.data_ptr(), self.u.data_ptr(), self.x.data_ptr(),
            self.pi_out.data_ptr(), self.lam_out.data_ptr(), self.t_out.data_ptr(), self.inf_norm_res.data_ptr(),
            self._stream()), "hpmpc_mi355x_ocp_finish_batch")
        return dict(self._sized(dict(u=self.u, x=self.x, pi=self.pi_out, lam=self.lam_out, t=self.t_out)),
                    inf_norm_res=self.inf_norm_res, kk=self.kk, status=self.ret)

    def results(self, out=None) -> list:
        """finish()'s tensors on the host, one interface-form dict per problem (synchronises)."""
        out = self.finish() if out is None else out
        self.torch.cuda.synchronize(self.dev)
        host = {k: v.cpu().numpy() for k, v in out.items()}
        per = unflatten_problems(host, self.N, self.nx, self.nu, self.nb, self.ng, self.order, keys=OUT_KEYS)
        for p, r in enumerate(per):
            r.update(inf_norm_res=host["inf_norm_res"][p].copy(), kk=int(host["kk"][p]), status=int(host["status"][p]),
                     stat=self.stat[p, :5 * max(int(host["kk"][p]), 0)].cpu().numpy())
        return per

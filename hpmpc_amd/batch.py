"""Batched, device-resident front end of libhpmpc_mi355x.so (additive API).

A batch is ``nprob`` independent QPs that share stage sizes and box indices.  All arrays live in
HBM as problem-major torch tensors (torch is plumbing here: allocation, streams, events); the solve
itself is one launch of the HIP kernels through the library's C ABI:

    BAbt  (nprob, packB)   lib4 stage blocks, stage k at offB[k]      (d_ip2_res_hard.c pBAbt[k])
    RSQrq (nprob, packR)   lib4 stage blocks, stage k at offR[k]      (pQ[k])
    d     (nprob, N+1, 32) [lb (pnb) | ub (pnb)] per stage            (d[k])
    ux    (nprob, N+1, 16) variable order u..x                        (ux[k])
    pi    (nprob, N+1, 16) over x_{k+1}                               (pi[k])
    lam/t (nprob, N+1, 32) reference padded layout                    (lam[k] / t[k])
    ws    (nprob, ws_doubles) factor + persistent IPM iterate

There is no CPU fallback: constructing a solver without a GPU or without the built library raises.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

from .bindings import LIBPATH, check, lib, plan_args  # noqa: F401  (tests, tools and bench.py import LIBPATH from here)
from .device import DeviceSolver, tensor_ptr
from .ocp import OCPQP

kkt_lib = lib  # the batched KKT re-solve's calls are bound with every other one (hpmpc_amd.bindings)


class _Layout(C.Structure):
    _fields_ = [("BAbt_stride", C.c_longlong), ("RSQrq_stride", C.c_longlong),
                ("BAbt_off", C.POINTER(C.c_longlong)), ("RSQrq_off", C.POINTER(C.c_longlong)),
                ("BAbt_shared", C.POINTER(C.c_ubyte)), ("RSQrq_shared", C.POINTER(C.c_ubyte))]


def aliased_layout(qp: OCPQP):
    """The time-invariant / aliased device layout of a batch whose problems differ only in stage 0's BAbt block (its b
    row carries A x0 + b): every other stage block is the same in every problem, and every inner stage the same as
    stage 1 (the reference drivers' aliasing, test_problems/test_d_ip_hard.c:652-662).  Returns the packed arrays
    (BAbt: [shared inner block | stage 0 of problem 0 | stage 0 of problem 1 | ...], RSQrq: [stage 0 | inner | N],
    shared by all problems), the strides, the offsets and the shared flags of hpmpc_mi355x_layout.  Raises
    ValueError when the data do not alias that way."""
    N, P = qp.N, qp.batch
    for k in range(1, N):
        for a, b in ((qp.BAbt[k], qp.BAbt[1]), (qp.RSQrq[k], qp.RSQrq[1])):
            if a.shape != b.shape or not np.array_equal(a, b):
                raise ValueError(f"stage {k} is not stage 1's (time-invariant inner stages needed)")
    for arr in list(qp.BAbt[1:]) + list(qp.RSQrq):
        if not (arr == arr[:1]).all():
            raise ValueError("stage data other than BAbt_0 differ between problems")
    inner = qp.BAbt[1][0] if N > 1 else np.zeros(0)
    b0 = qp.BAbt[0]
    hB = np.concatenate([inner, b0.reshape(-1)])
    offB = np.array([inner.size] + [0] * (N - 1), dtype=np.int64)
    shB = np.array([0] + [1] * (N - 1), dtype=np.uint8)
    r0, r1, rN = qp.RSQrq[0][0], qp.RSQrq[1][0], qp.RSQrq[N][0]
    hR = np.concatenate([r0, r1, rN])
    offR = np.array([0] + [r0.size] * (N - 1) + [r0.size + r1.size], dtype=np.int64)
    shR = np.ones(N + 1, dtype=np.uint8)
    return hB, hR, int(b0.shape[1]), 0, offB, offR, shB, shR


def stage_offsets(qp: OCPQP):
    """Offsets (doubles) of every stage block inside one problem's packed BAbt / RSQrq arrays, and the
    packed lengths: stage k of BAbt at offB[k], of RSQrq at offR[k] (the reference's lib4 blocks, unchanged)."""
    N = qp.N
    offB = np.zeros(N, dtype=np.int64)
    offR = np.zeros(N + 1, dtype=np.int64)
    o = 0
    for k in range(N):
        offB[k] = o
        o += qp.BAbt[k].shape[-1]
    packB = o
    o = 0
    for k in range(N + 1):
        offR[k] = o
        o += qp.RSQrq[k].shape[-1]
    return offB, offR, packB, o


def pack_batch(qp: OCPQP):
    """Problem-major host arrays of a batched OCPQP: BAbt (nprob, packB), RSQrq (nprob, packR), d (nprob, N+1, 32)
    -- the layout BatchSolver keeps in HBM and hpmpc_amd.shard scatters."""
    N = qp.N
    hB = np.ascontiguousarray(np.concatenate([a for a in qp.BAbt], axis=1))
    hR = np.ascontiguousarray(np.concatenate([a for a in qp.RSQrq], axis=1))
    hd = np.zeros((qp.batch, N + 1, 32))
    for k in range(N + 1):
        n = qp.d[k].shape[1]
        hd[:, k, :n] = qp.d[k]
    return hB, hR, hd


def unpack_batch(template: OCPQP, hB, hR, hd) -> OCPQP:
    """Inverse of pack_batch: the batched OCPQP whose stage sizes / idxb are the template's and whose data are
    the packed arrays (numpy or CPU tensors)."""
    hB, hR, hd = (np.asarray(x) for x in (hB, hR, hd))
    offB, offR, _, _ = stage_offsets(template)
    N = template.N
    BAbt = [hB[:, offB[k]:offB[k] + template.BAbt[k].shape[-1]].copy() for k in range(N)]
    RSQrq = [hR[:, offR[k]:offR[k] + template.RSQrq[k].shape[-1]].copy() for k in range(N + 1)]
    d = [hd[:, k, :template.d[k].shape[-1]].copy() for k in range(N + 1)]
    return OCPQP(N, template.nx.copy(), template.nu.copy(), template.nb.copy(), template.ng.copy(),
                 [i.copy() for i in template.idxb], BAbt, RSQrq, d, [], hB.shape[0])


def kkt_scratch_doubles(N: int) -> int:
    """Doubles of scratch one right-hand-side set of the batched KKT re-solve needs: six 16-double and four
    32-double vectors per stage (KKT_SCRATCH_V16 / _V32 of csrc/hk_kkt_args.h; hpmpc_mi355x_kkt_scratch_doubles)."""
    return (N + 1) * (6 * 16 + 4 * 32)


def kkt_buffers(torch, dev, plan, N: int, nprob: int, nrhs: int) -> dict:
    """Outputs and scratch of hpmpc_mi355x_kkt_new_rhs_batch for ``nrhs`` sets per problem: ux, pi (nprob, nrhs, N+1,
    16), lam, t (nprob, nrhs, N+1, 32), scratch (nprob, nrhs, hpmpc_mi355x_kkt_scratch_doubles)."""
    f64 = torch.float64
    new = lambda *shape: torch.zeros((nprob, nrhs) + shape, dtype=f64, device=dev)
    return dict(ux=new(N + 1, 16), pi=new(N + 1, 16), lam=new(N + 1, 32), t=new(N + 1, 32),
                scratch=new(int(lib().hpmpc_mi355x_kkt_scratch_doubles(plan))))


_OUT_WIDTH = dict(ux=16, pi=16, lam=32, t=32)


def _set_call(fn, torch, plan, layout, N, nprob, p0, count, nsets, BAbt, RSQrq, DCt, inputs, outs, out, ws,
              *tail) -> int:
    """A call with the argument list the set calls share -- plan, layout, range, nsets, the lib4 arrays, the per-set
    inputs, the per-set outputs, ws, scratch, then ``tail`` -- on torch tensors.  ``inputs``: rows (name, tensor,
    width, optional) of (nprob, nsets, N+1, width) tensors on the device of ``ws``, checked by tensor_ptr; ``outs``:
    the keys of ``out`` (from kkt_buffers(nsets)) in the call's order, None for an output passed as null.  Returns the
    library's code."""
    shape, dev = {16: (nprob, nsets, N + 1, 16), 32: (nprob, nsets, N + 1, 32)}, ws.device
    ins = [tensor_ptr(torch, x, shape[w], dev, name, optional) for name, x, w, optional in inputs]
    for name in outs:
        if name is not None and out[name].shape != shape[_OUT_WIDTH[name]]:
            raise ValueError(f"out[{name!r}]: buffers of kkt_buffers(nrhs={nsets}) expected")
    return fn(plan, layout, nprob, p0, count, nsets, BAbt.data_ptr(), RSQrq.data_ptr(),
              None if DCt is None else DCt.data_ptr(), *ins,
              *[None if name is None else out[name].data_ptr() for name in outs], ws.data_ptr(),
              out["scratch"].data_ptr(), *tail)


def kkt_sets_call(torch, plan, layout, N, nprob, p0, count, nrhs, BAbt, RSQrq, DCt, b, q, d, out, ws, compute_mult,
                  stream) -> int:
    """hpmpc_mi355x_kkt_new_rhs_batch on torch tensors, after checking the per-set arrays: b, q (nprob, nrhs, N+1, 16)
    or None (the problem's augmented rows), d (nprob, nrhs, N+1, 32), ``out`` from kkt_buffers.  Returns the library's
    code."""
    return _set_call(lib().hpmpc_mi355x_kkt_new_rhs_batch, torch, plan, layout, N, nprob, p0, count, nrhs, BAbt, RSQrq,
                     DCt, (("b", b, 16, True), ("q", q, 16, True), ("d", d, 32, False)), ("ux", "pi", "lam", "t"), out,
                     ws, compute_mult, stream)


def kkt_tangent_call(torch, plan, layout, N, nprob, p0, count, ndir, BAbt, RSQrq, DCt, db, dq, dd, out, ws,
                     compute_mult, stream) -> int:
    """hpmpc_mi355x_kkt_tangent_batch on torch tensors, after checking the per-set arrays: db, dq (nprob, ndir, N+1,
    16), dd (nprob, ndir, N+1, 32), each or all None (a zero direction); ``out`` from kkt_buffers(ndir), whose ux / pi /
    lam / t receive dux / dpi / dlam / dt.  Returns the library's code."""
    return _set_call(lib().hpmpc_mi355x_kkt_tangent_batch, torch, plan, layout, N, nprob, p0, count, ndir, BAbt, RSQrq,
                     DCt, (("db", db, 16, True), ("dq", dq, 16, True), ("dd", dd, 32, True)), ("ux", "pi", "lam", "t"),
                     out, ws, compute_mult, stream)


def kkt_adjoint_call(torch, plan, layout, N, nprob, p0, count, nadj, BAbt, RSQrq, DCt, gux, gpi, glam, gt, out, ws,
                     want_b, stream) -> int:
    """hpmpc_mi355x_kkt_adjoint_batch on torch tensors, after checking the per-set cotangents: gux, gpi (nprob, nadj,
    N+1, 16), glam, gt (nprob, nadj, N+1, 32), each or all None (zero); ``out`` from kkt_buffers(nadj), whose pi / ux /
    lam receive bbar / qbar / dbar (bbar only with ``want_b``; its t is not touched).  Returns the library's code."""
    return _set_call(lib().hpmpc_mi355x_kkt_adjoint_batch, torch, plan, layout, N, nprob, p0, count, nadj, BAbt, RSQrq,
                     DCt, (("gux", gux, 16, True), ("gpi", gpi, 16, True), ("glam", glam, 32, True),
                           ("gt", gt, 32, True)), ("pi" if want_b else None, "ux", "lam"), out, ws, stream)


class BatchSolver(DeviceSolver):
    """Device-resident batch of OCP QPs + the batched HPMPC entry points.

    ``nprob`` given: the batch's data are not uploaded from ``qp`` (which then only supplies stage sizes and
    idxb); BAbt / RSQrq / d are allocated for ``nprob`` problems and filled by the caller, e.g. by the rank-0
    scatter of hpmpc_amd.shard."""

    _destroy = "hpmpc_mi355x_plan_destroy"

    def __init__(self, qp: OCPQP, device="cuda", k_max: int = 50, nprob: int | None = None, aliased: bool = False):
        super().__init__(device)
        assert nprob is not None or qp.batch is not None, "BatchSolver takes a batched OCPQP"
        torch = self.torch
        self.qp = qp
        self.N = N = qp.N
        self.nprob = qp.batch if nprob is None else int(nprob)
        self.k_max = k_max
        L = lib()
        (nx, nu, nb, ng), idxp, self._keep = plan_args(qp.idxb, qp.nx, qp.nu, qp.nb, qp.ng)
        self.plan = L.hpmpc_mi355x_plan_create(N, nx, nu, nb, idxp, ng)
        if not self.plan:
            raise ValueError(f"unsupported problem sizes for the GPU path (code {L.hpmpc_mi355x_last_error()})")
        # problem-major packed inputs
        f64 = torch.float64
        P = self.nprob
        self.aliased = aliased
        if aliased:  # one copy of every shared stage block (hpmpc_mi355x_layout BAbt_shared / RSQrq_shared)
            assert nprob is None
            hB, hR, sB, sR, offB, offR, shB, shR = aliased_layout(qp)
            self.offB, self.offR, self._sh = offB, offR, (shB, shR)
            u8 = C.POINTER(C.c_ubyte)
            self.layout = _Layout(sB, sR, offB.ctypes.data_as(C.POINTER(C.c_longlong)),
                                  offR.ctypes.data_as(C.POINTER(C.c_longlong)), shB.ctypes.data_as(u8),
                                  shR.ctypes.data_as(u8))
            self.BAbt = torch.from_numpy(hB).to(self.dev)
            self.RSQrq = torch.from_numpy(hR).to(self.dev)
            self.d = torch.from_numpy(pack_batch(qp)[2]).to(self.dev)
        else:
            offB, offR, packB, packR = stage_offsets(qp)
            self.offB, self.offR = offB, offR
            self.layout = _Layout(packB, packR, offB.ctypes.data_as(C.POINTER(C.c_longlong)),
                                  offR.ctypes.data_as(C.POINTER(C.c_longlong)), None, None)
        if aliased:
            pass
        elif nprob is None:
            hB, hR, hd = pack_batch(qp)
            self.BAbt = torch.from_numpy(hB).to(self.dev)
            self.RSQrq = torch.from_numpy(hR).to(self.dev)
            self.d = torch.from_numpy(hd).to(self.dev)
        else:
            self.BAbt = torch.zeros((P, packB), dtype=f64, device=self.dev)
            self.RSQrq = torch.zeros((P, packR), dtype=f64, device=self.dev)
            self.d = torch.zeros((P, N + 1, 32), dtype=f64, device=self.dev)
        self.ux = torch.zeros((P, N + 1, 16), dtype=f64, device=self.dev)
        self.pi = torch.zeros((P, N + 1, 16), dtype=f64, device=self.dev)
        self.lam = torch.zeros((P, N + 1, 32), dtype=f64, device=self.dev)
        self.t = torch.zeros((P, N + 1, 32), dtype=f64, device=self.dev)
        self.Pb = torch.zeros((P, N + 1, 16), dtype=f64, device=self.dev)
        self.wsd = int(L.hpmpc_mi355x_ws_doubles(self.plan))
        self.ws = torch.zeros((P, self.wsd), dtype=f64, device=self.dev)
        self.kk = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.ret = torch.zeros(P, dtype=torch.int32, device=self.dev)
        self.stat = torch.zeros((P, 5 * k_max), dtype=f64, device=self.dev)

    def _ipm(self, name, p0, count, opts, *tail):
        """hpmpc_mi355x_<name> on problems [p0, p0 + count) with the arguments every batched IPM call shares
        (opts: mu0, mu_tol, alpha_min, warm_start, compute_mult), then ``tail`` and torch's current stream."""
        count = self.nprob - p0 if count is None else count
        p = lambda x: x.data_ptr()
        name = "hpmpc_mi355x_" + name
        check(getattr(lib(), name)(
            self.plan, C.byref(self.layout), self.nprob, p0, count, p(self.BAbt), p(self.RSQrq), p(self.d), p(self.ux),
            p(self.pi), p(self.lam), p(self.t), p(self.ws), self.k_max, *opts, p(self.kk), p(self.ret), p(self.stat),
            *tail, self._stream()), name)

    def ipm(self, *, mu0=2.0, mu_tol=1e-12, alpha_min=1e-8, warm_start=0, compute_mult=1, p0=0, count=None):
        """Batched d_ip2_res_mpc_hard_tv (asynchronous on torch's current stream)."""
        self._ipm("ipm_batch", p0, count, (mu0, mu_tol, alpha_min, warm_start, compute_mult))

    def ipm_solo(self, *, mu0=2.0, mu_tol=1e-12, alpha_min=1e-8, warm_start=0, compute_mult=1, p0=0, count=None):
        """ipm() as the latency path: each problem's whole solve in one launch (hpmpc_mi355x_ipm_solo)."""
        self._ipm("ipm_solo", p0, count, (mu0, mu_tol, alpha_min, warm_start, compute_mult))

    def kkt_buffers(self, nrhs: int = 1) -> dict:
        """The output and scratch tensors kkt_new_rhs(nrhs=nrhs) writes (allocated on first use, then reused)."""
        return self._per_set("kkt", nrhs, lambda n: kkt_buffers(self.torch, self.dev, self.plan, self.N, self.nprob, n))

    def kkt_new_rhs(self, b, q, d, nrhs=1, p0=0, count=None, compute_mult=1):
        """Batched d_kkt_solve_new_rhs_res_mpc_hard_tv on the factor ipm() / ipm_solo() left in ws (at least one
        iteration done; not after a queue solve): ``nrhs`` right-hand-side sets per problem in one launch.  b, q:
        (nprob, nrhs, N+1, 16) device tensors (b in state order, q in variable order [r | q]) or None for the
        problem's own rows; d: (nprob, nrhs, N+1, 32).  Returns ux, pi, lam, t with a leading (nprob, nrhs) shape --
        the tensors of kkt_buffers(nrhs), overwritten by the next call.  ws and the problem data are not written.
        A tensor that is not on the solver's device is refused with ValueError before the library is called.
        Asynchronous on torch's current stream."""
        p0, count = self._range(p0, count)
        out = self.kkt_buffers(nrhs)
        check(kkt_sets_call(self.torch, self.plan, C.byref(self.layout), self.N, self.nprob, p0, count, nrhs, self.BAbt,
                            self.RSQrq, None, b, q, d, out, self.ws, compute_mult, self._stream()),
              "hpmpc_mi355x_kkt_new_rhs_batch")
        return out["ux"], out["pi"], out["lam"], out["t"]

    def kkt_tangent(self, db, dq, dd, ndir=1, p0=0, count=None, compute_mult=1, out=None):
        """Batched KKT tangent solve (hpmpc_mi355x_kkt_tangent_batch): the directional derivative of kkt_new_rhs's
        result with respect to (b, q, d), ``ndir`` direction sets per problem in one launch, on the factor ipm() /
        ipm_solo() left.  db, dq: (nprob, ndir, N+1, 16), dd: (nprob, ndir, N+1, 32), or None for a zero direction.
        Returns dux, dpi, dlam, dt with a leading (nprob, ndir) shape: the tensors of ``out`` (default: those of
        kkt_buffers(ndir), which the next kkt_new_rhs / kkt_tangent call of that set count overwrites).  ws and the
        problem data are not written.  A direction that is not on the solver's device is refused with ValueError
        before the library is called.  Asynchronous on torch's current stream."""
        p0, count = self._range(p0, count)
        out = self.kkt_buffers(ndir) if out is None else out
        check(kkt_tangent_call(self.torch, self.plan, C.byref(self.layout), self.N, self.nprob, p0, count, ndir,
                               self.BAbt, self.RSQrq, None, db, dq, dd, out, self.ws, compute_mult, self._stream()),
              "hpmpc_mi355x_kkt_tangent_batch")
        return out["ux"], out["pi"], out["lam"], out["t"]

    def kkt_adjoint(self, gux, gpi, glam, gt, nadj=1, p0=0, count=None, want_b=True, out=None):
        """Batched KKT adjoint solve (hpmpc_mi355x_kkt_adjoint_batch): the transpose of kkt_tangent, ``nadj`` cotangent
        sets per problem in one launch, on the factor ipm() / ipm_solo() left.  gux, gpi: (nprob, nadj, N+1, 16), glam,
        gt: (nprob, nadj, N+1, 32), the cotangents of kkt_new_rhs's ux, pi, lam, t, or None for zero.  Returns (bbar,
        qbar, dbar), the gradients with respect to b, q and d, with a leading (nprob, nadj) shape: the pi, ux and lam
        tensors of ``out`` (default: those of kkt_buffers(nadj), which the next kkt_new_rhs / kkt_tangent /
        kkt_adjoint call of that set count overwrites).  want_b=False skips the multiplier half of the solve and
        returns bbar as None.  ws and the problem data are not written.  A cotangent that is not on the solver's device
        is refused with ValueError before the library is called.  Asynchronous on torch's current stream."""
        p0, count = self._range(p0, count)
        out = self.kkt_buffers(nadj) if out is None else out
        check(kkt_adjoint_call(self.torch, self.plan, C.byref(self.layout), self.N, self.nprob, p0, count, nadj,
                               self.BAbt, self.RSQrq, None, gux, gpi, glam, gt, out, self.ws, want_b, self._stream()),
              "hpmpc_mi355x_kkt_adjoint_batch")
        return (out["pi"] if want_b else None), out["ux"], out["lam"]

    def ipm_pass(self, pss, *, mu0=2.0, mu_tol=1e-12, alpha_min=1e-8, warm_start=0, compute_mult=1, p0=0,
                 count=None):
        """One pass of the batched IPM (0 init, 1 factorisation, 2 predictor, 3 corrector, 4 update);
        ipm() == pass 0 then k_max rounds of passes 1..4."""
        self._ipm("ipm_pass", p0, count, (mu0, mu_tol, alpha_min, warm_start, compute_mult), pss)

    def ipm_profiled(self, *, mu0=2.0, mu_tol=1e-12, alpha_min=1e-8, warm_start=0, compute_mult=1):
        """ipm() with hipEvents around every pass kernel (synchronous).  Returns the summed device time
        (ms) of passes [init, factorisation, predictor, corrector, update]."""
        out = np.zeros(5)
        self._ipm("ipm_batch_profiled", 0, None, (mu0, mu_tol, alpha_min, warm_start, compute_mult), out.ctypes.data)
        return out

    def queue(self, nq: int, n_slots: int | None = None) -> "IpmQueue":
        """A continuous-batching IPM over this batch's data (entry q solves problem q % nprob)."""
        return IpmQueue(self, nq, self.nprob if n_slots is None else n_slots)

    def ric_sv(self, *, compute_pi=1, compute_Pb=0, p0=0, count=None):
        """Batched d_back_ric_rec_sv_tv_res (nb = ng = 0, no update rows): factor into ws."""
        count = self.nprob - p0 if count is None else count
        check(lib().hpmpc_mi355x_ric_sv_batch(
            self.plan, C.byref(self.layout), self.nprob, p0, count, self.BAbt.data_ptr(), self.RSQrq.data_ptr(),
            self.ux.data_ptr(), self.pi.data_ptr(), self.ws.data_ptr(), compute_pi, compute_Pb,
            self.Pb.data_ptr(), self._stream()), "hpmpc_mi355x_ric_sv_batch")

    def ric_sv_bound(self, stream=None, *, compute_pi=1, compute_Pb=0):
        """ric_sv over the whole batch as a zero-argument callable with every argument marshalled once (a stream
        handle, or the current stream at bind time): a launch loop then costs one foreign call per launch.  The
        callable returns the library's code (0 on success)."""
        fn = lib().hpmpc_mi355x_ric_sv_batch
        st = C.c_void_p(self.torch.cuda.current_stream(self.dev).cuda_stream if stream is None else stream.cuda_stream)
        args = (self.plan, C.byref(self.layout), self.nprob, 0, self.nprob, C.c_void_p(self.BAbt.data_ptr()),
                C.c_void_p(self.RSQrq.data_ptr()), C.c_void_p(self.ux.data_ptr()), C.c_void_p(self.pi.data_ptr()),
                C.c_void_p(self.ws.data_ptr()), compute_pi, compute_Pb, C.c_void_p(self.Pb.data_ptr()), st)
        return lambda: fn(*args)

    def ric_trf(self, *, p0=0, count=None):
        """Batched d_back_ric_rec_trf_tv_res (nb = ng = 0): factor into ws."""
        count = self.nprob - p0 if count is None else count
        check(lib().hpmpc_mi355x_ric_trf_batch(self.plan, C.byref(self.layout), self.nprob, p0, count,
                                               self.BAbt.data_ptr(), self.RSQrq.data_ptr(), self.ws.data_ptr(),
                                               self._stream()), "hpmpc_mi355x_ric_trf_batch")

    def ric_trs(self, b, q, *, compute_pi=1, compute_Pb=1, p0=0, count=None):
        """Batched d_back_ric_rec_trs_tv_res with the factor left in ws by ric_sv."""
        count = self.nprob - p0 if count is None else count
        check(lib().hpmpc_mi355x_ric_trs_batch(
            self.plan, C.byref(self.layout), self.nprob, p0, count, self.BAbt.data_ptr(), self.RSQrq.data_ptr(),
            b.data_ptr(), q.data_ptr(), self.ux.data_ptr(), self.pi.data_ptr(), self.ws.data_ptr(), compute_pi,
            compute_Pb, self.Pb.data_ptr(), self._stream()), "hpmpc_mi355x_ric_trs_batch")


def algorithmic_bytes_per_ip_iter(qp: OCPQP) -> float:
    """Algorithmic HBM bytes of one residual-based IP iteration of one problem:
    sv = BAbt + lower(RSQrq)+row read, L lower+row+inv_diag written, ux/pi written;
    trs = L + BAbt re-read, rhs (q, b) in, (ux, pi) out; res = lower(RSQrq) + BAbt re-read, ux/pi in,
    r_q/r_b out; IPM box vectors 24 doubles per box."""
    tot = 0
    N = qp.N
    for k in range(N + 1):
        nux = qp.nux(k)
        nx1 = int(qp.nx[k + 1]) if k < N else 0
        T = nux * (nux + 1) // 2
        babt = (nux + 1) * nx1
        rsq = T + nux
        L = T + 2 * nux
        sv = babt + rsq + L + nux + nx1
        trs = L + babt + (nux + nx1) + (nux + nx1)
        res = rsq + babt + (nux + nx1) + (nux + nx1)
        tot += sv + trs + res + 24 * int(qp.nb[k])
    return 8.0 * tot


def algorithmic_bytes_per_fact(qp: OCPQP) -> float:
    """Algorithmic HBM bytes of one problem through the IPM factorisation pass (hk_ipm_fact, phase 2,
    residuals fused): BAbt (with its b row) and lower(RSQrq)+q row read, the iterate ux / pi read and
    the residuals r_q / r_b written, box vectors lam, t, r_m, r_d read and t_inv written (10 doubles
    per box), factor L lower + row + inv_diag and P b written."""
    tot = 0
    N = qp.N
    for k in range(N + 1):
        nux = qp.nux(k)
        nx1 = int(qp.nx[k + 1]) if k < N else 0
        T = nux * (nux + 1) // 2
        tot += (nux + 1) * nx1 + (T + nux) + 2 * (nux + nx1) + 10 * int(qp.nb[k]) + (T + 2 * nux) + nx1
    return 8.0 * tot


def algorithmic_bytes_per_pass(qp: OCPQP) -> dict:
    """Algorithmic HBM bytes of one problem-iteration through each IPM pass kernel (phase 2), each datum
    counted once per pass, T = nux(nux+1)/2, per box pair (lower + upper):
    - hk_ipm_fact: algorithmic_bytes_per_fact;
    - hk_ipm_pred: factor L (T + 2 nux), BAbt with r_b in place of its b row; boxes r_d, lam, t read and
      dt, dlam written (10); the step itself is not stored;
    - hk_ipm_corr (trs + forward): L, BAbt + r_b, r_q (nux), stored P b (nx'), ux (nux) and pi (nx')
      written; boxes t, dt, dlam, lam, r_d read, r_m, dt, dlam written (16);
    - hk_ipm_update (queue API: no backups, no r_m store -- nothing in a queue solve reads them): ux, dux
      read, ux written (3 nux), the same for pi (3 nx'); boxes lam, t, dlam, dt, d read, lam, t, r_d
      written (16);
    - hk_ipm_predcorr (the queue's launch of both): hk_ipm_pred + hk_ipm_corr."""
    out = {"hk_ipm_fact": algorithmic_bytes_per_fact(qp), "hk_ipm_pred": 0.0, "hk_ipm_corr": 0.0,
           "hk_ipm_update": 0.0, "hk_ipm_predcorr": 0.0}
    N = qp.N
    for k in range(N + 1):
        nux = qp.nux(k)
        nx1 = int(qp.nx[k + 1]) if k < N else 0
        nb = int(qp.nb[k])
        T = nux * (nux + 1) // 2
        L = T + 2 * nux
        babt = (nux + 1) * nx1
        out["hk_ipm_pred"] += 8.0 * (L + babt + 10 * nb)
        out["hk_ipm_corr"] += 8.0 * (L + babt + nux + nx1 + nux + nx1 + 16 * nb)
        out["hk_ipm_update"] += 8.0 * (3 * nux + 3 * nx1 + 16 * nb)
    out["hk_ipm_predcorr"] = out["hk_ipm_pred"] + out["hk_ipm_corr"]  # the queue's fused launch: both passes' data
    return out


def algorithmic_bytes_per_sv(qp: OCPQP) -> float:
    """8 N [(nux+1)nx' + (T+nux) + (T+2nux) + nux + nx'] (sum over stages)."""
    tot = 0
    N = qp.N
    for k in range(N + 1):
        nux = qp.nux(k)
        nx1 = int(qp.nx[k + 1]) if k < N else 0
        T = nux * (nux + 1) // 2
        tot += (nux + 1) * nx1 + (T + nux) + (T + 2 * nux) + nux + nx1
    return 8.0 * tot


def flops_sv(N, nx, nu):
    """Reference flop count of one sv (test_problems/test_d_ric_mpc.c:578-590), compute_pi included."""
    return ((1 / 3) * nx ** 3 + 1.5 * nx ** 2) + N * ((7 / 3) * nx ** 3 + 4 * nx ** 2 * nu + 2 * nx * nu ** 2 +
                                                    (1 / 3) * nu ** 3 + 6.5 * nx ** 2 + 9 * nx * nu + 2.5 * nu ** 2) \
        - (nx * (nx + nu) + (1 / 3) * nx ** 3 + 1.5 * nx ** 2) + N * 2 * nx ** 2


def flops_ip_iter(N, nx, nu):
    trs = N * (6 * nx ** 2 + 8 * nx * nu + 2 * nu ** 2) + N * 2 * nx ** 2
    res = N * (2 * (nx + nu) ** 2 + 4 * (nx + nu) * nx)
    return flops_sv(N, nx, nu) + trs + res


QUEUE_LANES_MAX = 4  # include/hpmpc_mi355x.h HPMPC_MI355X_QUEUE_LANES_MAX


class IpmQueue:
    """Problem queue over a BatchSolver's data (hpmpc_mi355x_ipm_queue): ``nq`` entries solved by
    ``n_slots`` resident slots; a slot whose problem has finished takes the next entry at the next
    iteration.  Iterates and outputs are per entry, workspaces per slot.  From 2048 slots up the queue runs as
    lanes on their own streams (one per 1024 slots, at most 4; HPMPC_MI355X_QUEUE_LANES) that hand out entries
    from one shared counter, joined back into the caller's stream at the end."""

    def __init__(self, solver: BatchSolver, nq: int, n_slots: int):
        torch = solver.torch
        self.s = solver
        self.nq, self.n_slots = int(nq), int(n_slots)
        N, f64, dev = solver.N, torch.float64, solver.dev
        self.ux = torch.zeros((nq, N + 1, 16), dtype=f64, device=dev)
        self.pi = torch.zeros((nq, N + 1, 16), dtype=f64, device=dev)
        self.lam = torch.zeros((nq, N + 1, 32), dtype=f64, device=dev)
        self.t = torch.zeros((nq, N + 1, 32), dtype=f64, device=dev)
        self.kk = torch.zeros(nq, dtype=torch.int32, device=dev)
        self.ret = torch.zeros(nq, dtype=torch.int32, device=dev)
        self.stat = torch.zeros((nq, 5 * solver.k_max), dtype=f64, device=dev)
        self.ws = torch.zeros((n_slots, solver.wsd), dtype=f64, device=dev)
        # HPMPC_MI355X_QUEUE_CTL_INTS (include/hpmpc_mi355x.h): up to QUEUE_LANES_MAX lane blocks + drain counters
        self.qctl = torch.zeros(6 * QUEUE_LANES_MAX + 2 + 3 * n_slots, dtype=torch.int32, device=dev)

    def lanes(self):
        """The lane split of hpmpc_mi355x_ipm_queue (the C driver's rule): [(control-block offset in qctl, slots)]
        per lane; HPMPC_MI355X_QUEUE_LANES lanes (default 4), at most one per 1024 slots.  The lanes hand out entries
        from one shared counter."""
        L = int(os.environ.get("HPMPC_MI355X_QUEUE_LANES", "4"))
        L = max(1, min(L, self.n_slots // 1024, QUEUE_LANES_MAX, self.nq, self.n_slots))
        out, s0 = [], 0
        for i in range(L):
            ns = self.n_slots // L + (i < self.n_slots % L)
            out.append((6 * i + 3 * s0, ns))
            s0 += ns
        return out

    def finished(self):
        """Entries finished in the last run, over every lane (read after a synchronise)."""
        return sum(int(self.qctl[o + 1].item()) for o, _ in self.lanes())

    def idle(self):
        """Whether every slot of every lane was left without an entry (read after a synchronise)."""
        return all(bool((self.qctl[o + 2:o + 2 + ns] == -1).all()) for o, ns in self.lanes())

    def drained(self):
        """(iterations, problems) the multi-wave drain finished in the last run (read after a synchronise)."""
        o = 6 * QUEUE_LANES_MAX + 3 * self.n_slots
        return int(self.qctl[o].item()), int(self.qctl[o + 1].item())

    # what pass_ms[i] of run(profiled=True) times (include/hpmpc_mi355x.h): a tick is hk_ipm_fact, hk_ipm_predcorr
    # (predictor and corrector back to back) and hk_ipm_update; [3] stays 0
    PASS_KERNELS = ("hk_ipm_init + hk_ipm_qdrain_mw", "hk_ipm_fact", "hk_ipm_predcorr", None, "hk_ipm_update")

    def run(self, *, mu0=2.0, mu_tol=1e-12, alpha_min=1e-8, warm_start=0, compute_mult=1, profiled=False):
        """Solve every entry.  Returns (pass_ms[5] or None, ticks): see PASS_KERNELS.  Polls the device once per
        chunk; the caller synchronises before reading results."""
        s = self.s
        out = np.zeros(5)
        ticks = C.c_int(0)
        rc = lib().hpmpc_mi355x_ipm_queue(
            s.plan, C.byref(s.layout), s.nprob, self.nq, self.n_slots, s.BAbt.data_ptr(), s.RSQrq.data_ptr(),
            s.d.data_ptr(), self.ux.data_ptr(), self.pi.data_ptr(), self.lam.data_ptr(), self.t.data_ptr(),
            self.ws.data_ptr(), self.qctl.data_ptr(), s.k_max, mu0, mu_tol, alpha_min, warm_start, compute_mult,
            self.kk.data_ptr(), self.ret.data_ptr(), self.stat.data_ptr(), out.ctypes.data if profiled else None,
            C.byref(ticks), s._stream())
        check(rc, "hpmpc_mi355x_ipm_queue")
        return (out if profiled else None), ticks.value

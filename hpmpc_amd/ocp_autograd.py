"""The batched OCP solve as a differentiable torch layer: ``ocp_solve(solver, data)`` runs OcpBatchSolver's pack ->
solve -> finish and its backward is one OcpBatchSolver.adjoint_data call (hpmpc_mi355x_ocp_adjoint_data_batch: the KKT
adjoint solve hk_kkt_adj, then the matrix gradients hk_ocp_matgrad); under torch.autograd.forward_ad its jvp is one
OcpBatchSolver.tangent_data call (hpmpc_mi355x_ocp_tangent_data_batch: the matrix directions hk_ocp_matdir, then the
KKT tangent solve hk_kkt_tan).  torch is plumbing here; every direction is a HIP kernel and there is no CPU fallback.
"""
from __future__ import annotations

from .ocp_batch import KEYS, OUT_KEYS


def _function():
    """The autograd.Function, built on first use so that importing this module does not import torch."""
    global _OcpSolve
    if _OcpSolve is not None:
        return _OcpSolve
    import torch
    from torch.autograd.function import once_differentiable

    class OcpSolve(torch.autograd.Function):
        @staticmethod
        def forward(ctx, solver, keys, mu0, mu_tol, alpha_min, *tensors):
            solver.pack({key: x.detach() for key, x in zip(keys, tensors)})
            solver.solve(mu0=mu0, mu_tol=mu_tol, alpha_min=alpha_min)
            out = solver.finish()
            ctx.solver, ctx.keys = solver, keys
            ctx.shared = [x.dim() == 1 for x in tensors]
            ctx.token = solver._autograd_token = object()
            ctx.set_materialize_grads(False)
            return tuple(out[key].clone() for key in OUT_KEYS)

        @staticmethod
        @once_differentiable
        def backward(ctx, *gouts):
            sv = ctx.solver
            if getattr(sv, "_autograd_token", None) is not ctx.token:
                raise RuntimeError("ocp_solve: the solver ran another ocp_solve since this forward; its factor and "
                                   "iterate are gone")
            needs = ctx.needs_input_grad[5:]
            want = tuple(key for key, need in zip(ctx.keys, needs) if need)
            grads = [None] * len(ctx.keys)
            if want:
                cot = {key: g.contiguous().reshape(sv.nprob, 1, g.shape[-1]) for key, g in zip(OUT_KEYS, gouts)
                       if g is not None}
                got = sv.adjoint_data(cot, 1, want=want)
                for i, (key, need, shared) in enumerate(zip(ctx.keys, needs, ctx.shared)):
                    if need:  # the buffers are the solver's and are overwritten by its next call
                        grads[i] = got[key][:, 0].sum(0) if shared else got[key][:, 0].clone()
            return (None, None, None, None, None, *grads)

        @staticmethod
        def jvp(ctx, *tins):
            sv = ctx.solver
            if getattr(sv, "_autograd_token", None) is not ctx.token:
                raise RuntimeError("ocp_solve: the solver ran another ocp_solve since this forward; its factor and "
                                   "iterate are gone")
            dirs = {}
            for key, t, shared in zip(ctx.keys, tins[5:], ctx.shared):
                if t is not None:  # a shared tensor's tangent moves every problem's array
                    t = t.detach()
                    dirs[key] = (t.expand(sv.nprob, -1) if shared else t).reshape(sv.nprob, 1, -1).contiguous()
            got = sv.tangent_data(dirs, 1)
            return tuple(got[key][:, 0].clone() for key in OUT_KEYS)  # the buffers are the solver's

    _OcpSolve = OcpSolve
    return OcpSolve


_OcpSolve = None


def ocp_solve(solver, data, mu0=2.0, mu_tol=1e-10, alpha_min=1e-8):
    """Solve the batch of ``solver`` (an OcpBatchSolver) for the dense ``data`` ({key: tensor (nprob, size), or (size,)
    for an array shared by every problem}, as for OcpBatchSolver.pack) and return ``(u, x, pi, lam, t)``, the tensors of
    OcpBatchSolver.finish() (cloned), differentiable with respect to every tensor of ``data`` that requires a gradient.
    ``kk`` and ``status`` stay on the solver (solver.kk, solver.ret).

    Backward builds one cotangent set from the incoming gradients (an output without one is left out of the set) and
    calls solver.adjoint_data(..., 1, want=the keys whose tensors need a gradient).  Every such tensor receives a
    gradient of its own shape: (nprob, size), or for a shared (size,) tensor the sum over the problems; the others
    receive None.  Q and R receive the gradient for symmetric perturbations; the blocks of a time-invariant matrix are
    separate inputs here and their gradients are not summed over the stages.

    Forward mode (torch.autograd.forward_ad): the tangents of the five outputs are one solver.tangent_data(..., 1) on
    the tangents of the inputs that have one -- a shared (size,) tensor's tangent is expanded over the problems, an
    input without a tangent does not move; Q and R act through the symmetric parts of their tangents.  One solve gives
    the derivative of the whole plan along one parameter direction, where backward takes one per output element.

    What is differentiated, in both modes: the linearised KKT system on the factor solve() persisted -- the re-solve's
    tangent in the vectors and the matrix tangent defined in include/hpmpc_mi355x.h (forward), and their exact
    transposes (backward) -- at the raw iterate,
    without finish()'s equality-box fix.  That factor belongs to the last Newton system of the IPM, formed one iterate
    before the returned point, so this is not the derivative of a fully converged solve: finite differences of whole
    solves agree to about 1e-3 relative, and torch.autograd.gradcheck is the wrong test for it.  Problems with
    status != 0 get whatever that system gives.  Double backward is not supported.  The solver keeps the factor and
    the iterate: do not solve other data with it between this call and its backward."""
    keys = tuple(key for key in KEYS if data.get(key) is not None)
    return _function().apply(solver, keys, mu0, mu_tol, alpha_min, *(data[key] for key in keys))

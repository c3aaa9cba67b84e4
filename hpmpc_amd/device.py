"""What the device-resident solver classes share (BatchSolver, OcpBatchSolver, SoftBatchSolver, PcondSolver): the one
check a caller's tensor passes before its pointer reaches the library, and the scaffolding around a plan handle.  torch
is passed in, so importing this module loads neither torch nor the library.
"""
from __future__ import annotations

from .bindings import lib


def tensor_ptr(torch, x, shape, dev, what, optional=False):
    """``x.data_ptr()`` of a float64 tensor that is contiguous, of exactly ``shape`` and on ``dev`` (a resolved device,
    e.g. that of a tensor the solver owns: "cuda" and "cuda:0" are then one device); None for a missing ``optional``
    one.  Anything else is a ValueError: a host pointer, or one into another GPU's memory, must not reach a kernel."""
    if x is None:
        if optional:
            return None
    elif x.dtype == torch.float64 and x.shape == tuple(shape) and x.device == dev and x.is_contiguous():
        return x.data_ptr()
    raise ValueError(f"{what}: contiguous float64 tensor of shape {tuple(shape)} on {dev} expected")


class DeviceSolver:
    """Base of the solver classes: refuses to exist without a GPU, holds ``torch`` and the resolved device ``dev``, and
    destroys ``self.plan`` with the library call the subclass names in ``_destroy``."""

    _destroy = None  # name of the library's *_plan_destroy for self.plan

    def __init__(self, device):
        import torch

        if not torch.cuda.is_available():
            raise RuntimeError(f"{type(self).__name__} needs a GPU (HIP device); there is no CPU fallback")
        self.torch = torch
        self.dev = torch.empty(0, device=device).device  # resolved: "cuda" becomes the current device's "cuda:<i>"

    def __del__(self):
        try:
            if getattr(self, "plan", None):
                getattr(lib(), self._destroy)(self.plan)
        except Exception:
            pass

    def _stream(self):
        return self.torch.cuda.current_stream(self.dev).cuda_stream

    def _range(self, p0, count):
        return p0, (self.nprob - p0 if count is None else count)

    def _tensor(self, x, shape, what, optional=False):
        return tensor_ptr(self.torch, x, shape, self.dev, what, optional)

    def _per_set(self, kind, n, make):
        """The buffers ``make(n)`` of ``kind`` for ``n`` sets per problem: allocated on first use, then that object."""
        if n < 1:
            raise ValueError("at least one set per problem expected")
        cache = self.__dict__.setdefault("_set_buffers", {})
        if (kind, n) not in cache:
            cache[kind, n] = make(n)
        return cache[kind, n]

"""The one ctypes binding of libhpmpc_mi355x.so's batched API (Part 2 of include/hpmpc_mi355x.h): the library path,
the loader, the signature of every ``hpmpc_mi355x_*`` function and the marshalling helpers the solver classes share.

``SIGNATURES`` is checked against the header by tests/test_bindings_host.py, prototype by prototype, so an argument
list that drifts from the C side fails a CPU test instead of handing a pointer to a kernel as an int.
"""
from __future__ import annotations

import ctypes as C
import os

import numpy as np

# HPMPC_MI355X_LIB: another build of the same library (A/B timing of two builds on one box, tools/gpu_ab.sh)
LIBPATH = os.environ.get("HPMPC_MI355X_LIB") or os.path.join(os.path.dirname(os.path.abspath(__file__)), "lib",
                                                             "libhpmpc_mi355x.so")

_CTYPE = dict(v=None, i=C.c_int, d=C.c_double, l=C.c_longlong, p=C.c_void_p, s=C.c_char_p)
# "<return>:<arguments>" in the header's order: v void, i int, d double, l long long, p any pointer, s const char *
_SIG = dict(
    plan_create="p:ippppp",
    plan_destroy="v:p",
    ws_doubles="l:p",
    ipm_batch="i:ppiiippppppppidddiipppp",
    ipm_solo="i:ppiiippppppppidddiipppp",
    ipm_pass="i:ppiiippppppppidddiipppip",
    ipm_batch_profiled="i:ppiiippppppppidddiippppp",
    ipm_queue="i:ppiiipppppppppidddiipppppp",
    ric_sv_batch="i:ppiiipppppiipp",
    ric_trf_batch="i:ppiiipppp",
    ric_trs_batch="i:ppiiipppppppiipp",
    last_error="i:",
    version="s:",
    pcond_plan_create="p:ipppppi",
    pcond_plan_destroy="v:p",
    pcond_sizes="i:pp",
    pcond_offsets="i:pip",
    pcond_batch="i:piiippppppppp",
    pcond_ric_sv_batch="i:piiipppppip",
    pexpand_batch="i:piiippppppppppp",
    wide_plan_create="p:ippppp",
    wide_plan_destroy="v:p",
    wide_sizes="i:pp",
    wide_offsets="i:pp",
    wide_ipm_batch="i:piiipppppppppidddiipppp",
    pcond_wide_plan="p:p",
    soft_plan_create="p:ipppppp",
    soft_plan_destroy="v:p",
    soft_sizes="i:pp",
    soft_offsets="i:pp",
    ipm_soft_batch="i:ppiiippppppppppidddiipppp",
    ocp_plan_create="p:ipppppi",
    ocp_plan_destroy="v:p",
    ocp_tile_plan="p:p",
    ocp_sizes="i:pp",
    ocp_offsets="i:pp",
    ocp_pack_batch="i:ppiiiipppppppp",
    ocp_ipm_batch="i:piiipppppppppidddiipppp",
    ocp_finish_batch="i:piiipppppppppppppppp",
    ocp_soft_plan_create="p:ippppppi",
    ocp_soft_plan_destroy="v:p",
    ocp_soft_ipm_plan="p:p",
    ocp_soft_sizes="i:pp",
    ocp_soft_offsets="i:pp",
    ocp_soft_pack_batch="i:ppiiiippppppppp",
    ocp_soft_ipm_batch="i:piiippppppppppidddiipppp",
    ocp_soft_finish_batch="i:piiippppppppppppppppp",
    soft_kkt_scratch_doubles="l:p",
    soft_kkt_batch="i:ppiiiippppppppppppppppiip",
    soft_kkt_ocp_work_doubles="l:p",
    soft_kkt_ocp_batch="i:piiiippppppppppppppppppppip",
    kkt_scratch_doubles="l:p",
    kkt_new_rhs_batch="i:ppiiiippppppppppppip",
    ocp_kkt_batch="i:piiippppppppppp",
    ocp_unpack_sets="i:piiiippppppppppp",
    kkt_tangent_batch="i:ppiiiippppppppppppip",
    ocp_tangent_batch="i:ppiiiippppppppppip",
    kkt_adjoint_batch="i:ppiiiippppppppppppp",
    ocp_adjoint_batch="i:piiiipppppppppppppppppp",
    ocp_matrix_grads_batch="i:piiiipppppppp",
    ocp_adjoint_data_batch="i:piiiippppppppppppppp",
    ocp_matrix_dirs_batch="i:ppiiiippppppp",
    ocp_tangent_data_batch="i:ppiiiipppppppppppppip",
)
# {function name: (restype, argtypes)}
SIGNATURES = {"hpmpc_mi355x_" + n: (_CTYPE[s[0]], [_CTYPE[c] for c in s[2:]]) for n, s in _SIG.items()}

_LIB = None


def bind(L):
    """Declare every function of SIGNATURES that ``L`` has; one it lacks is skipped, so an A/B library from before
    that call (HPMPC_MI355X_LIB) still loads for everything else."""
    for name, (restype, argtypes) in SIGNATURES.items():
        fn = getattr(L, name, None)
        if fn is not None:
            fn.restype, fn.argtypes = restype, argtypes
    return L


def lib() -> C.CDLL:
    """Load the in-tree HIP library (raises if it was not built)."""
    global _LIB
    if _LIB is None:
        if not os.path.exists(LIBPATH):
            raise RuntimeError(f"libhpmpc_mi355x.so not built ({LIBPATH}); run __graft_entry__.build()")
        _LIB = bind(C.CDLL(LIBPATH, mode=os.RTLD_LOCAL | getattr(os, "RTLD_NOW", 2)))
    return _LIB


def check(rc: int, name: str) -> None:
    if rc != 0:
        raise RuntimeError(f"{name} failed ({rc})")


def plan_args(idxb, *sizes):
    """The size arguments of a *_plan_create call: (addresses of the int32 copies of ``sizes``, the int** of the
    per-stage ``idxb`` rows, the objects that keep both alive)."""
    ints = lambda a: np.ascontiguousarray(a, dtype=np.int32)
    arrs, idx = [ints(a) for a in sizes], [ints(a) for a in idxb]
    idxp = (C.POINTER(C.c_int) * len(idx))(*[a.ctypes.data_as(C.POINTER(C.c_int)) for a in idx])
    return [a.ctypes.data for a in arrs], C.cast(idxp, C.c_void_p), (arrs, idx, idxp)

"""Host-side checks of the batched KKT re-solve (no GPU): the numpy helpers that build the per-set b / q / d arrays,
the C interface (header, export list, built library) and the scratch carve."""
import ctypes as C
import fnmatch
import os
import re
import sys

import numpy as np
import pytest

from hpmpc_amd import batch
from hpmpc_amd.cabi import bq_from_qp
from hpmpc_amd.ocp_batch import kkt_set_arrays
from ocp_batch_cases import CASES, problems

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "oracle"))
import iface_oracle as IO  # noqa: E402

ENTRY_POINTS = ("hpmpc_mi355x_kkt_scratch_doubles", "hpmpc_mi355x_kkt_new_rhs_batch", "hpmpc_mi355x_ocp_kkt_batch")


@pytest.mark.parametrize("case", ["V", "S", "H", "E", "B"])
def test_set_arrays_match_the_oracle_helpers(case):
    """b, q against hpmpc_amd.cabi.bq_from_qp of the packed problem and d against to_qp's d, element for element;
    everything beyond them (the padding of the 16- / 32-double stage slots, b at stage N) is zero."""
    base = problems(case, range(3))
    Ps = base + [IO.new_rhs(P, seed=6 + i) for i, P in enumerate(base)]
    b, q, d = kkt_set_arrays(Ps)
    N = CASES[case][0]
    assert b.shape == q.shape == (len(Ps), N + 1, 16) and d.shape == (len(Ps), N + 1, 32)
    for p, P in enumerate(Ps):
        qp = IO.to_qp(P)
        bb, qq = bq_from_qp(qp)
        for k in range(N + 1):
            want_b = np.zeros(16)
            if k < N:
                n = min(16, bb[k].size)
                want_b[:n] = bb[k][:n]
                assert not bb[k][n:].any()
            want_q, want_d = np.zeros(16), np.zeros(32)
            n = min(16, qq[k].size)
            want_q[:n] = qq[k][:n]
            assert not qq[k][n:].any()
            want_d[:min(32, qp.d[k].size)] = qp.d[k][:32]
            assert np.array_equal(b[p, k], want_b), (p, k)
            assert np.array_equal(q[p, k], want_q), (p, k)
            assert np.array_equal(d[p, k], want_d), (p, k)
    assert b.any() and q.any() and d.any()
    with pytest.raises(ValueError):
        kkt_set_arrays([Ps[0], problems("F", [0])[0]])  # one batch, one set of stage sizes


def test_entry_points_declared_and_exported():
    header = open(os.path.join(ROOT, "include", "hpmpc_mi355x.h")).read()
    code = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    exports = open(os.path.join(ROOT, "hpmpc_amd", "csrc", "exports.map")).read()
    globs = re.findall(r"^\s*([\w\*]+);", exports.split("global:")[1].split("local:")[0], flags=re.M)
    for name in ENTRY_POINTS:
        assert re.search(r"\b%s\s*\(" % name, code), name
        assert any(fnmatch.fnmatchcase(name, g) for g in globs), (name, globs)
        assert name in exports, name  # named in the list's description too
    # the prototypes the issue fixed: nrhs after count, ws const, scratch before compute_mult
    proto = re.search(r"int hpmpc_mi355x_kkt_new_rhs_batch\((.*?)\);", code, flags=re.S).group(1)
    args = [a.strip().split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert args == ["plan", "lay", "nprob", "p0", "count", "nrhs", "BAbt", "RSQrq", "DCt", "b", "q", "d", "ux", "pi",
                    "lam", "t", "ws", "scratch", "compute_mult", "stream"], args
    assert re.search(r"const double \*ws", proto)
    proto = re.search(r"int hpmpc_mi355x_ocp_kkt_batch\((.*?)\);", code, flags=re.S).group(1)
    args = [a.strip().split()[-1].lstrip("*") for a in proto.replace("\n", " ").split(",")]
    assert args == ["plan", "nprob", "p0", "count", "BAbt", "RSQrq", "DCt", "d", "ux", "pi", "lam", "t", "ws",
                    "scratch", "stream"], args
    assert "#define HPMPC_MI355X_OCP_NSIZES 29" in header  # unchanged


def test_library_has_the_entry_points():
    if not os.path.exists(batch.LIBPATH):
        from hpmpc_amd.build import build_hip

        build_hip()
    lib = C.CDLL(batch.LIBPATH, mode=os.RTLD_LOCAL)
    for name in ENTRY_POINTS:
        assert hasattr(lib, name), name
    # the size query needs no device: a null plan has no scratch
    lib.hpmpc_mi355x_kkt_scratch_doubles.restype = C.c_longlong
    lib.hpmpc_mi355x_kkt_scratch_doubles.argtypes = [C.c_void_p]
    assert lib.hpmpc_mi355x_kkt_scratch_doubles(None) == 0


def test_scratch_size_is_the_kernel_headers_carve():
    """6 V16 + 4 V32 vectors per stage: the constants of csrc/hk_kkt_args.h, the strides of csrc/hpmpc_kargs.h and
    the Python formula agree (the library's own value is compared with the formula on the GPU, where a plan exists)."""
    csrc = os.path.join(ROOT, "hpmpc_amd", "csrc")
    args = open(os.path.join(csrc, "hk_kkt_args.h")).read()
    kargs = open(os.path.join(csrc, "hpmpc_kargs.h")).read()
    const = lambda text, name: int(re.search(r"constexpr int %s = (\d+);" % name, text).group(1))
    n16, n32 = const(args, "KKT_SCRATCH_V16"), const(args, "KKT_SCRATCH_V32")
    v16, v32 = const(kargs, "V16"), const(kargs, "V32")
    assert (n16, n32, v16, v32) == (6, 4, 16, 32)
    assert "(N + 1) * (KKT_SCRATCH_V16 * V16 + KKT_SCRATCH_V32 * V32)" in args
    for N in (1, 5, 100):
        assert batch.kkt_scratch_doubles(N) == (N + 1) * (n16 * v16 + n32 * v32)
        assert batch.kkt_scratch_doubles(N) % 32 == 0  # whole 256-byte granules: the sets stay line-aligned
    # the kernel's carve uses every vector it declares, once
    kern = open(os.path.join(csrc, "hk_kkt.hip")).read()
    carved = re.findall(r"w\.(\w+) = S", kern)
    assert sorted(carved) == sorted(["res_q", "res_b", "qx", "dux", "dpi", "Pb", "res_d", "res_m", "dt", "dlam"])

"""A tensor that is not on the solver's device never reaches the library: every set call of BatchSolver and
OcpBatchSolver refuses it with ValueError first (hpmpc_amd.device.tensor_ptr).

The library functions behind the calls are replaced by recorders that return 0, so nothing is launched whichever way the
check goes: a refusal that came too late would show as a recorded call, not as a kernel reading host memory."""
import pytest

from hpmpc_amd.bindings import lib
from ocp_batch_cases import make_solver, problems
from test_gpu_kkt_batch import _batched_qp

pytestmark = pytest.mark.gpu
NPROB, NSETS = 2, 2
RECORDED = ("kkt_new_rhs_batch", "kkt_tangent_batch", "kkt_adjoint_batch", "ocp_tangent_batch", "ocp_adjoint_batch",
            "ocp_matrix_grads_batch", "ocp_adjoint_data_batch")


def test_a_host_tensor_is_refused_before_the_library_is_called():
    import torch

    from hpmpc_amd.batch import BatchSolver

    Ps = problems("S", range(NPROB))
    bs = BatchSolver(_batched_qp(Ps), k_max=1)
    sv = make_solver(Ps, "C", k_max=1)
    N, s = sv.N, sv.sizes
    assert (bs.nprob, sv.nprob, s["b"]) == (NPROB, NPROB, 2)
    pad = {w: (NPROB, NSETS, N + 1, w) for w in (16, 32)}
    osz = dict(u=s["u"], x=s["x"], pi=s["pi_out"], lam=s["lam_out"], t=s["lam_out"])
    dense = lambda sizes: {key: (NPROB, NSETS, n) for key, n in sizes.items()}
    vec = {key: s[key] for key in ("b", "q", "r", "lb", "ub", "lg", "ug")}
    base = {key: (NPROB, s[key]) for key in ("ux", "pi", "lam")}

    def tensors(shapes, host):
        """float64 zeros of ``shapes`` on the solver's device, the one at index / key ``host`` on the CPU"""
        new = lambda k, shape: torch.zeros(shape, dtype=torch.float64, device="cpu" if k == host else sv.dev)
        if isinstance(shapes, dict):
            return {k: new(k, shape) for k, shape in shapes.items()}
        return [new(k, shape) for k, shape in enumerate(shapes)]

    p16, p32 = pad[16], pad[32]
    # (library function, the call on a tensor list / dict, the shapes, the indices / keys handed over as CPU tensors)
    calls = [
        ("kkt_new_rhs_batch", lambda t: bs.kkt_new_rhs(*t, nrhs=NSETS), [p16, p16, p32], range(3)),
        ("kkt_tangent_batch", lambda t: bs.kkt_tangent(*t, ndir=NSETS), [p16, p16, p32], range(3)),
        ("kkt_adjoint_batch", lambda t: bs.kkt_adjoint(*t, nadj=NSETS), [p16, p16, p32, p32], range(4)),
        ("kkt_new_rhs_batch", lambda t: sv.kkt_sets(*t, nrhs=NSETS), [p16, p16, p32], range(3)),
        ("kkt_tangent_batch", lambda t: sv.tangent_sets(*t, ndir=NSETS), [p16, p16, p32], range(3)),
        ("kkt_adjoint_batch", lambda t: sv.adjoint_sets(*t, nadj=NSETS), [p16, p16, p32, p32], range(4)),
        ("ocp_tangent_batch", lambda t: sv.tangent(t, NSETS), dense(vec), list(vec)),
        ("ocp_adjoint_batch", lambda t: sv.adjoint(t, NSETS), dense(osz), list(osz)),
        ("ocp_adjoint_data_batch", lambda t: sv.adjoint_data(t, NSETS), dense(osz), list(osz)),
        ("ocp_adjoint_data_batch", lambda t: sv.adjoint_data(tensors(dense(osz), None), NSETS, base=t), base,
         list(base)),
        ("ocp_matrix_grads_batch", lambda t: sv.matrix_gradients(*t, NSETS), [p16, p16, p32], range(3)),
        ("ocp_matrix_grads_batch", lambda t: sv.matrix_gradients(*tensors([p16, p16, p32], None), NSETS, base=t), base,
         list(base)),
    ]
    L = lib()
    saved = {name: getattr(L, "hpmpc_mi355x_" + name) for name in RECORDED}
    seen = []
    try:
        for name in RECORDED:
            setattr(L, "hpmpc_mi355x_" + name, lambda *args, _name=name: seen.append(_name) or 0)
        for name, call, shapes, hosts in calls:
            del seen[:]
            call(tensors(shapes, None))  # the recorder stands where the call goes: device tensors reach it
            assert seen == [name], (name, seen)
            for host in hosts:
                del seen[:]
                with pytest.raises(ValueError):
                    call(tensors(shapes, host))
                assert seen == [], (name, host, seen)
    finally:
        for name, fn in saved.items():
            setattr(L, "hpmpc_mi355x_" + name, fn)
    assert all(getattr(L, "hpmpc_mi355x_" + name) is fn for name, fn in saved.items())

"""The differentiable OCP layer (hpmpc_amd.ocp_autograd.ocp_solve) on the GPU: forward is pack -> solve -> finish,
backward is one OcpBatchSolver.adjoint_data call.  What adjoint_data computes is checked against the oracle in
tests/test_gpu_kkt_matgrad.py; here the layer's plumbing is checked against adjoint_data itself, bit for bit.  No test
uses torch.autograd.gradcheck: it compares with finite differences of whole solves, which agree with the linearised
KKT system on the persisted factor only to about 1e-3 (include/hpmpc_mi355x.h).
"""
import numpy as np
import pytest

import kkt_tangent_cases as TC
import test_gpu_kkt_batch as KB
from hpmpc_amd.ocp_batch import KEYS, OUT_KEYS, flatten_problems
from ocp_batch_cases import make_solver, problems, to_device

pytestmark = pytest.mark.gpu
CASE, SEEDS = "V", (0, 1, 2, 3)


def _bits(x):
    return np.ascontiguousarray(x.detach().cpu().numpy()).view(np.int64)


def _same(a, b):
    return a.shape == b.shape and np.array_equal(_bits(a), _bits(b))


def _setup(case):
    """(solver, the dense data tensors of the tightened problems, one random cotangent per output, the problems)"""
    from hpmpc_amd.ocp_autograd import ocp_solve  # noqa: F401  (the module imports without torch loaded by it)

    Ps = [KB.tighten(P) for P in problems(case, SEEDS)]
    sv = make_solver(Ps, "C")
    data = to_device(sv, flatten_problems(Ps, "C"))
    rng = np.random.default_rng(3)
    s = sv.sizes
    size = dict(u=s["u"], x=s["x"], pi=s["pi_out"], lam=s["lam_out"], t=s["lam_out"])
    cot = {k: sv.torch.from_numpy(rng.standard_normal((len(Ps), size[k]))).to(sv.dev) for k in OUT_KEYS}
    return sv, data, cot, Ps


@pytest.fixture(scope="module")
def setup():
    return _setup(CASE)


def _leaves(data, needs=KEYS):
    return {k: v.clone().requires_grad_(k in needs) for k, v in data.items()}


def _reference(sv, cot, want=KEYS, keys=OUT_KEYS):
    """adjoint_data of the cotangent on the solver's current state, copied out of its buffers"""
    got = sv.adjoint_data({k: cot[k][:, None].contiguous() for k in keys}, 1, want=want)
    return {k: v[:, 0].clone() for k, v in got.items()}


def test_forward_is_pack_solve_finish(setup):
    from hpmpc_amd.ocp_autograd import ocp_solve

    sv, data, _, Ps = setup
    out = ocp_solve(sv, _leaves(data), **TC.TIGHT)
    assert len(out) == 5 and all(x.requires_grad for x in out)
    fin = sv.finish()
    for key, x in zip(OUT_KEYS, out):
        assert x.data_ptr() != fin[key].data_ptr() and _same(x, fin[key]), key
    assert sv.ret.tolist() == [0] * len(SEEDS) and min(sv.kk.tolist()) >= 1
    # the same by hand on a second solver
    sv2 = make_solver(Ps, "C")
    sv2.pack(data)
    sv2.solve(**TC.TIGHT)
    fin2 = sv2.finish()
    for key, x in zip(OUT_KEYS, out):
        assert _same(x, fin2[key]), key
    assert sv2.kk.tolist() == sv.kk.tolist()


def _backward_is_adjoint_data(setup):
    from hpmpc_amd.ocp_autograd import ocp_solve

    sv, data, cot, _ = setup
    leaves = _leaves(data)
    out = ocp_solve(sv, leaves, **TC.TIGHT)
    loss = sum((x * cot[k]).sum() for k, x in zip(OUT_KEYS, out))  # a random linear loss: d loss / d out = cot
    loss.backward()
    ref = _reference(sv, cot)
    for key in KEYS:
        g = leaves[key].grad
        assert g is not None and g.shape == data[key].shape and _same(g, ref[key]), key
    assert min(float(leaves[key].grad.abs().max()) for key in KEYS) > 1e-6


def test_backward_is_adjoint_data_bit_for_bit(setup):
    _backward_is_adjoint_data(setup)


def test_backward_is_adjoint_data_bit_for_bit_at_the_tile_edge():
    """Case E: 16 x 16 blocks of A and Q, 16 rows of C, nu = 0 on an inner stage -- the largest arrays the layer sees.
    A test of its own, so that the V test keeps its id."""
    _backward_is_adjoint_data(_setup("E"))


def test_shared_input_gets_the_sum_over_problems(setup):
    from hpmpc_amd.ocp_autograd import ocp_solve

    sv, data, cot, _ = setup
    shared = dict(data, A=data["A"][0].clone())  # one A for every problem
    leaves = _leaves(shared, needs=("A", "b"))
    out = ocp_solve(sv, leaves, **TC.TIGHT)
    sv.torch.autograd.backward(out, [cot[k] for k in OUT_KEYS])
    ref = _reference(sv, cot, want=("A", "b"))
    assert leaves["A"].grad.shape == shared["A"].shape and _same(leaves["b"].grad, ref["b"])
    # a sum of nprob terms in float64: 4 roundings of the absolute sum, whatever the order
    want, bound = ref["A"].sum(0), 4 * np.finfo(np.float64).eps * ref["A"].abs().sum(0)
    assert bool(((leaves["A"].grad - want).abs() <= bound).all()) and float(want.abs().max()) > 1e-3
    per = _reference(sv, cot, want=("A",))["A"].cpu().numpy()
    assert np.abs(per[0] - per[1]).max() > 1e-6  # the problems' gradients differ: the sum is not a copy


def test_inputs_without_requires_grad_get_none(setup):
    from hpmpc_amd.ocp_autograd import ocp_solve

    sv, data, cot, _ = setup
    needs = ("Q", "r", "C")
    leaves = _leaves(data, needs=needs)
    out = ocp_solve(sv, leaves, **TC.TIGHT)
    sv.torch.autograd.backward(out, [cot[k] for k in OUT_KEYS])
    ref = _reference(sv, cot, want=needs)
    for key in KEYS:
        if key in needs:
            assert _same(leaves[key].grad, ref[key]), key
        else:
            assert leaves[key].grad is None, key
    # nothing needs a gradient: the outputs are plain tensors
    plain = ocp_solve(sv, data, **TC.TIGHT)
    assert not any(x.requires_grad for x in plain)


def test_missing_grad_outputs_act_as_zero(setup):
    from hpmpc_amd.ocp_autograd import ocp_solve

    sv, data, cot, _ = setup
    leaves = _leaves(data)
    out = ocp_solve(sv, leaves, **TC.TIGHT)
    (out[0] * cot["u"]).sum().backward()  # x, pi, lam, t receive no gradient at all
    ref = _reference(sv, cot, keys=("u",))
    zero = dict(cot, **{k: sv.torch.zeros_like(cot[k]) for k in OUT_KEYS if k != "u"})
    ref0 = _reference(sv, zero)
    for key in KEYS:
        assert _same(leaves[key].grad, ref[key]) and _same(ref[key], ref0[key]), key

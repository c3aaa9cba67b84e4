"""Forward-mode autograd of hpmpc_amd.ocp_autograd.ocp_solve on the GPU: under torch.autograd.forward_ad the tangents
of the five outputs are bit for bit OcpBatchSolver.tangent_data(..., 1) on the inputs' tangents; a shared 1-D input's
tangent moves every problem; inputs without a tangent are ignored."""
import numpy as np
import pytest

import kkt_matdir_cases as DC
import kkt_tangent_cases as TC
import test_gpu_kkt_tangent as TT
from hpmpc_amd.ocp_batch import OUT_KEYS, flatten_problems
from ocp_batch_cases import make_solver, to_device

pytestmark = pytest.mark.gpu
_same = TT._same


@pytest.fixture(scope="module")
def refs(oracle):
    return DC.shared(oracle)


def _setup(refs, case, n):
    seeds = refs.usable(case)[:n]
    Ps = [refs.ipm(case, s)[0] for s in seeds]
    sv = make_solver(Ps, "C")
    return sv, Ps, to_device(sv, flatten_problems(Ps, sv.order))


def _tangents(sv, data, keys, seed):
    rng = np.random.default_rng(seed)
    return {k: sv.torch.from_numpy(rng.standard_normal(tuple(data[k].shape))).to(sv.dev) for k in keys}


def _jvp(sv, data, tans):
    import torch.autograd.forward_ad as fwAD

    from hpmpc_amd.ocp_autograd import ocp_solve

    with fwAD.dual_level():
        dual = {k: fwAD.make_dual(x, tans[k]) if k in tans else x for k, x in data.items()}
        outs = ocp_solve(sv, dual, **TC.TIGHT)
        pairs = [fwAD.unpack_dual(o) for o in outs]
        return [p.primal.clone() for p in pairs], [None if p.tangent is None else p.tangent.clone() for p in pairs]


def _jvp_is_tangent_data(refs, case):
    sv, Ps, data = _setup(refs, case, 4)
    keys = ("A", "B", "Q", "R", "C", "D", "b", "q", "lb", "ug")  # S, r, ub, lg: no tangent, they do not move
    tans = _tangents(sv, data, keys, 3)
    primal, tangent = _jvp(sv, data, tans)
    want = sv.tangent_data({k: t.reshape(sv.nprob, 1, -1).contiguous() for k, t in tans.items()}, 1)
    sv.torch.cuda.synchronize()
    for key, p, t in zip(OUT_KEYS, primal, tangent):
        assert t is not None and t.shape == p.shape, key
        h = t.cpu().numpy()
        assert np.isfinite(h).all() and _same(h, want[key][:, 0].cpu().numpy()), key
    assert min(float(t.abs().max()) for t in tangent) > 1e-6
    # the primal is the ordinary solve
    out = sv.finish()
    for key, p in zip(OUT_KEYS, primal):
        assert _same(p.cpu().numpy(), out[key].cpu().numpy()), key


def test_jvp_is_bitwise_tangent_data(refs):
    _jvp_is_tangent_data(refs, "V")


def test_jvp_is_bitwise_tangent_data_at_the_tile_edge(refs):
    """Case E: 16 x 16 blocks of A and Q, 16 rows of C, nu = 0 on an inner stage -- the largest arrays the layer sees.
    A test of its own, so that the V test keeps its id."""
    _jvp_is_tangent_data(refs, "E")


def test_a_shared_input_and_inputs_without_tangent(refs):
    sv, Ps, data = _setup(refs, "F", 3)
    data = dict(data)
    data["Q"] = data["Q"][0].clone()  # one Q for every problem
    assert data["Q"].dim() == 1
    tans = _tangents(sv, data, ("Q", "b"), 5)
    primal, tangent = _jvp(sv, data, tans)
    dirs = {"Q": tans["Q"].expand(sv.nprob, -1).reshape(sv.nprob, 1, -1).contiguous(),
            "b": tans["b"].reshape(sv.nprob, 1, -1).contiguous()}
    want = sv.tangent_data(dirs, 1)
    for key, t in zip(OUT_KEYS, tangent):
        assert _same(t.cpu().numpy(), want[key][:, 0].cpu().numpy()), key
    assert float(tangent[1].abs().max()) > 1e-6
    # a tangent on b alone: every other input is ignored, and it is the dense tangent call's result
    _, tb = _jvp(sv, data, {"b": tans["b"]})
    vec = sv.tangent({"b": dirs["b"]}, 1)
    for key, t in zip(OUT_KEYS, tb):
        assert _same(t.cpu().numpy(), vec[key][:, 0].cpu().numpy()), key

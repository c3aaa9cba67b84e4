"""Host-side checks (no GPU, no library) of hpmpc_amd.device -- the one tensor check every set call goes through and the
per-set-count buffer cache of the solver classes -- and of ocp_batch.flatten_sets against the numpy restatement it
replaced in the test helpers and the timing tools."""
import numpy as np
import pytest
import torch

from hpmpc_amd.device import DeviceSolver, tensor_ptr
from hpmpc_amd.ocp_batch import VEC_KEYS, flatten_sets, unflatten_problems
from kkt_tangent_cases import RSEED, delta_of
from ocp_batch_cases import IO, problems

CPU = torch.device("cpu")
SHAPE = (2, 3, 4)


def _good():
    return torch.zeros(SHAPE, dtype=torch.float64)


def test_tensor_ptr_accepts_a_conforming_tensor():
    x = _good()
    assert tensor_ptr(torch, x, SHAPE, CPU, "x") == x.data_ptr()
    assert tensor_ptr(torch, x, list(SHAPE), x.device, "x", optional=True) == x.data_ptr()


@pytest.mark.parametrize("bad", ["dtype", "strides", "shape", "missing"])
def test_tensor_ptr_refuses(bad):
    x = {"dtype": lambda: torch.zeros(SHAPE, dtype=torch.float32),
         "strides": lambda: torch.zeros((2, 4, 3), dtype=torch.float64).transpose(1, 2),
         "shape": lambda: torch.zeros((2, 3, 5), dtype=torch.float64),
         "missing": lambda: None}[bad]()
    if x is not None:
        assert tuple(x.shape) == SHAPE or bad == "shape"
        assert x.is_contiguous() or bad == "strides"
    with pytest.raises(ValueError):
        tensor_ptr(torch, x, SHAPE, CPU, "x")


def test_tensor_ptr_refuses_the_wrong_device():
    with pytest.raises(ValueError):
        tensor_ptr(torch, _good(), SHAPE, torch.device("cuda", 0), "x")
    with pytest.raises(ValueError):
        tensor_ptr(torch, _good(), SHAPE, torch.device("cuda", 0), "x", optional=True)


def test_tensor_ptr_missing_optional_is_null():
    assert tensor_ptr(torch, None, SHAPE, CPU, "x", optional=True) is None
    assert tensor_ptr(torch, None, SHAPE, torch.device("cuda", 0), "x", optional=True) is None


def test_per_set_cache():
    sv = DeviceSolver.__new__(DeviceSolver)  # the cache needs neither a GPU nor a plan
    made = []

    def make(n):
        made.append(n)
        return dict(n=n)

    a = sv._per_set("kkt", 2, make)
    assert sv._per_set("kkt", 2, make) is a and made == [2]
    b = sv._per_set("kkt", 3, make)
    assert b is not a and b == dict(n=3)
    assert sv._per_set("sets", 2, make) is not a  # another kind with the same count is another entry
    assert sv._per_set("kkt", 2, make) is a and made == [2, 3, 2]
    for n in (0, -1):
        with pytest.raises(ValueError):
            sv._per_set("kkt", n, make)
    assert made == [2, 3, 2]


def _delta_sets(case, nprob=3, nsets=2):
    Ps = problems(case, range(nprob))
    return Ps, [[delta_of(P, IO.new_rhs(P, seed=RSEED + r)) for r in range(nsets)] for P in Ps]


@pytest.mark.parametrize("case", ["V", "V0", "F", "S"])
def test_flatten_sets_is_the_concatenated_stage_blocks(case):
    Ps, sets = _delta_sets(case)
    got = flatten_sets(sets, 2, VEC_KEYS)
    assert tuple(got) == VEC_KEYS
    for key in VEC_KEYS:
        want = np.array([[np.concatenate([np.ravel(np.asarray(v, dtype=np.float64)) for v in D[key]] + [np.zeros(0)])
                          for D in row] for row in sets], dtype=np.float64).reshape(3, 2, -1)
        assert got[key].dtype == np.float64 and got[key].shape == want.shape, key
        assert np.array_equal(got[key], want), key
    assert any(np.any(got[key] != 0) for key in VEC_KEYS)


@pytest.mark.parametrize("case", ["V", "V0", "F", "S"])
def test_flatten_sets_round_trips(case):
    Ps, sets = _delta_sets(case)
    P = Ps[0]
    flat = flatten_sets(sets, 2, VEC_KEYS)
    back = unflatten_problems({key: v.reshape(3 * 2, -1) for key, v in flat.items()}, P["N"], P["nx"], P["nu"],
                              P["nb"], P["ng"], keys=list(VEC_KEYS))
    assert len(back) == 6
    for i, D in enumerate(D for row in sets for D in row):
        for key in VEC_KEYS:
            blocks = back[i][key]
            assert len(blocks) >= len(D[key]), key
            for k, blk in enumerate(blocks):  # unflatten_problems pads r with stage N's empty block
                want = np.asarray(D[key][k], dtype=np.float64) if k < len(D[key]) else np.zeros(0)
                assert np.array_equal(blk, want), (i, key, k)

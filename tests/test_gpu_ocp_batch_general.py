"""General constraints over a batch: hpmpc_mi355x_ocp_ipm_batch with ng > 0 and nprob > 1, the one configuration of
the IPM pass kernels (hk_ipm_init / _fact / _pred / _corr / _update with KArgs.DCt and a problem stride sG) that no
other test runs -- the existing batched calls refuse ng > 0, and the reference-named entry points solve one problem.
Case V with its ng = [0, 0, 2, 0, 3, 2], three problems, both orders, against IO.ip_ocp over the CPU oracle at the
gates of tests/test_gpu_iface.py (identical status and kk, u / x / pi / lam / t at TOL_IPM, inf_norm_res at 1e-9);
every problem has oracle status 0 (asserted)."""
import numpy as np
import pytest

from ocp_batch_cases import check, expected_packed, oracle_ref, packed_host, problems, solve_batch

pytestmark = pytest.mark.gpu
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def refs(oracle):
    Ps = problems("V", SEEDS)
    return Ps, [oracle_ref(oracle, P) for P in Ps]


@pytest.mark.parametrize("order", ["C", "F"])
def test_general_constraints_over_a_batch(refs, order):
    Ps, ref = refs
    assert all(r["status"] == 0 for r in ref)
    assert sum(Ps[0]["ng"]) == 7
    sv, got = solve_batch(Ps, order)
    packed = packed_host(sv)
    for p, P in enumerate(Ps):  # the DCt blocks the solve read are to_qp's
        assert np.array_equal(packed["DCt"][p], expected_packed(sv, P)["DCt"]), p
    for p, (g, r) in enumerate(zip(got, ref)):
        check(g, r, tag=(order, p))

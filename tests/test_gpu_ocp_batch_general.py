"""General constraints over a batch: hpmpc_mi355x_ocp_ipm_batch with ng > 0 and nprob > 1, the one configuration of
the IPM pass kernels (hk_ipm_init / _fact / _pred / _corr / _update with KArgs.DCt and a problem stride sG) that no
other test runs -- the existing batched calls refuse ng > 0, and the reference-named entry points solve one problem.
Case V with its ng = [0, 0, 2, 0, 3, 2] and case E with ng = [12, 7, 8, 8, 16] (the 16-wide tile edge), three problems
each, both orders, against IO.ip_ocp over the CPU oracle at the gates of tests/test_gpu_iface.py (identical status and
kk, u / x / pi / lam / t at TOL_IPM, inf_norm_res at 1e-9); every problem has oracle status 0 (asserted)."""
import numpy as np
import pytest

from ocp_batch_cases import check, expected_packed, oracle_ref, packed_host, problems, solve_batch

pytestmark = pytest.mark.gpu
SEEDS = (1, 2, 3)


@pytest.fixture(scope="module")
def refs(oracle):
    """Problems and oracle solutions per case, computed once and shared (never modified)."""
    cache = {}

    def get(case):
        if case not in cache:
            Ps = problems(case, SEEDS)
            cache[case] = (Ps, [oracle_ref(oracle, P) for P in Ps])
        return cache[case]

    return get


def _batch(refs, case, order, ng_total):
    Ps, ref = refs(case)
    assert all(r["status"] == 0 for r in ref)
    assert sum(Ps[0]["ng"]) == ng_total
    sv, got = solve_batch(Ps, order)
    packed = packed_host(sv)
    for p, P in enumerate(Ps):  # the DCt blocks the solve read are to_qp's
        assert np.array_equal(packed["DCt"][p], expected_packed(sv, P)["DCt"]), p
    worst = max(check(g, r, tag=(case, order, p)) for p, (g, r) in enumerate(zip(got, ref)))
    print(case, order, "worst relative error of the solve", worst)


@pytest.mark.parametrize("order", ["C", "F"])
def test_general_constraints_over_a_batch(refs, order):
    _batch(refs, "V", order, 7)


@pytest.mark.parametrize("order", ["C", "F"])
def test_general_constraints_at_the_tile_edge(refs, order):
    """Case E: ng = [12, 7, 8, 8, 16], every stage's nb + ng slots filling the 16 of the tile (4 + 12, 8 + 8 with both
    padded, 8 + 8 on nu = 0, 8 + 8 on input boxes, 0 + 16 on the last stage), general constraints on stage 0 with a
    variable x_0."""
    _batch(refs, "E", order, 51)

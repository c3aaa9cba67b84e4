"""Time the OCP matrix gradients (hpmpc_mi355x_ocp_matrix_grads_batch / hpmpc_mi355x_ocp_adjoint_data_batch,
hk_matgrad.hip) beside the dense adjoint solve they follow (hpmpc_mi355x_ocp_adjoint_batch, hk_adj.hip).

    python tools/kkt_matgrad_time.py [--nprob 1024] [--distinct 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: that of tools/batch_time.py and tools/kkt_adjoint_time.py (N = 100, nx = 12, nu = 4, nx[0] = 0; `nprob`
problems, `distinct` different ones tiled to the batch).  One hpmpc_mi355x_ocp_ipm_batch leaves the factor.  Then, for
nadj = 1, 4 cotangent sets per problem (standard-normal cotangents on every element of u, x, pi, lam, t):
  adjoint_dense : OcpBatchSolver.adjoint, all seven vector gradients -- the call as it was before the matrix gradients,
                  the yardstick;
  adjoint_data  : OcpBatchSolver.adjoint_data, all fourteen gradients (hk_kkt_adj, then hk_ocp_matgrad);
  matgrad       : OcpBatchSolver.matrix_gradients alone on the padded adjoint solution, all seven matrices.
hipEvents around each call; per run the legs are called one after another (alternated in one process, so that clock and
thermal drift hit them alike), `warmup` such rounds, then the median, minimum and maximum of `runs`.  us per set, and
for matgrad GB/s against the bytes a set must move: per stage nx1 (nu + nx) + (nu + nx)^2 + ng (nu + nx) doubles
written and 128 read (the base iterate's 64 are shared by a problem's sets and counted once per set all the same).
Prints one JSON line.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_time import alternated, cotangent_tensors, cotangents, emit, parser, solved_batch  # noqa: E402

NADJ = (1, 4)


def matgrad_bytes(sv):
    """Bytes one set must move through hk_ocp_matgrad: every element of the seven dense gradients written, the stage's
    ux, pi, lam, qbar, bbar, dbar slots (128 doubles) read."""
    from hpmpc_amd.ocp_batch import MAT_KEYS

    return 8 * (sum(sv.sizes[key] for key in MAT_KEYS) + 128 * (sv.N + 1))


def main():
    a = parser().parse_args()
    import torch

    from hpmpc_amd.ocp_batch import KEYS, MAT_KEYS

    Ps, nd, sv, tile, out = solved_batch(torch, a, lambda sv: dict(matgrad=matgrad_bytes(sv)))
    cots = cotangents(np.random.default_rng(7), Ps, max(NADJ))
    for n in NADJ:
        cot, (gux, gpi, glam, gt) = cotangent_tensors(torch, sv, tile, Ps, cots, n)
        bbar, qbar, dbar = (x.clone() for x in sv.adjoint_sets(gux, gpi, glam, gt, n))
        t = alternated(torch, dict(adjoint_dense=lambda: sv.adjoint(cot, n),
                                   adjoint_data=lambda: sv.adjoint_data(cot, n),
                                   matgrad=lambda: sv.matrix_gradients(bbar, qbar, dbar, n)), a.warmup, a.runs)
        nsets = a.nprob * n
        for r in t.values():
            r.update(us_per_set=r["ms"] * 1e3 / nsets, spread_us_per_set=(r["ms_max"] - r["ms_min"]) * 1e3 / nsets)
        t["matgrad"]["GBps"] = out["bytes_per_set"]["matgrad"] * nsets / (t["matgrad"]["ms"] * 1e-3) / 1e9
        t["sets"] = nsets
        t["data_over_dense"] = t["adjoint_data"]["ms"] / t["adjoint_dense"]["ms"]
        t["excess_us_per_set"] = (t["adjoint_data"]["ms"] - t["adjoint_dense"]["ms"]) * 1e3 / nsets
        got = sv.adjoint_data(cot, n)
        t["finite"] = bool(all(torch.isfinite(got[key]).all().item() for key in KEYS))
        t["max_abs"] = {key: float(got[key].abs().max().item()) for key in MAT_KEYS if got[key].numel()}
        out[f"nadj{n}"] = t
        del cot, gux, gpi, glam, gt, bbar, qbar, dbar, got
    emit(out, a.out)


if __name__ == "__main__":
    main()

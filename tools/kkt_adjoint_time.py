"""Time the batched KKT adjoint solve (hpmpc_mi355x_kkt_adjoint_batch / hpmpc_mi355x_ocp_adjoint_batch, hk_adj.hip)
beside the tangent solve it is the transpose of (hk_tan.hip), at equal set counts, and the feedback gain by either.

    python tools/kkt_adjoint_time.py [--nprob 1024] [--distinct 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: that of tools/batch_time.py and tools/kkt_tangent_time.py (N = 100, nx = 12, nu = 4, nx[0] = 0; `nprob`
problems, `distinct` different ones tiled to the batch).  One hpmpc_mi355x_ocp_ipm_batch leaves the factor.  Then, for
nsets = 1, 8, 12 sets per problem:
  tangent       : OcpBatchSolver.tangent_sets with the directions new_rhs - problem (padded arrays), hk_kkt_tan;
  tangent_dense : OcpBatchSolver.tangent with the same directions as dense tensors;
  adjoint       : OcpBatchSolver.adjoint_sets with standard-normal cotangents on every element of u, x, pi, lam, t
                  (padded arrays), hk_kkt_adj;
  adjoint_dense : OcpBatchSolver.adjoint with the same cotangents as dense tensors, all seven gradients wanted.
And the gain d u_0 / d x_0 (nx0 = 12, nu[0] = 4) with random A0, S0:
  gain_tangent  : OcpBatchSolver.feedback_gain, 12 tangent sets per problem;
  gain_adjoint  : OcpBatchSolver.feedback_gain_adjoint, 4 adjoint sets per problem and the chain rule's two einsums.
hipEvents around each call; per run the legs are called one after another (alternated in one process, so that clock and
thermal drift hit them alike), `warmup` such rounds, then the median, minimum and maximum of `runs`.  us per set and
GB/s against the bytes a set must move (its problem's BAbt, RSQrq, DCt and factor once, its vectors in and out;
work-vector traffic not counted).  Prints one JSON line.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_time import (NX, alternated, cotangent_tensors, cotangents, direction_tensors, emit, parser,  # noqa: E402
                        rhs_sets, solved_batch)
from kkt_tangent_time import tangent_bytes  # noqa: E402

NSETS = (1, 8, 12)


def adjoint_bytes(sv):
    """Bytes one cotangent set must move: BAbt, RSQrq, DCt and the factor records read once, gux, gpi, glam, gt, t^-1
    and the multiplier backup read, qbar, bbar, dbar written (16- / 32-double stage slots)."""
    n1 = sv.N + 1
    s = sv.sizes
    return 8 * (s["BAbt"] + s["RSQrq"] + s["DCt"] + 352 * n1 + (2 * 16 + 2 * 32) * n1 + 2 * 32 * n1 +
                (2 * 16 + 32) * n1)


def main():
    a = parser().parse_args()
    import torch

    Ps, nd, sv, tile, out = solved_batch(torch, a,
                                         lambda sv: dict(tangent=tangent_bytes(sv), adjoint=adjoint_bytes(sv)))
    deltas = rhs_sets(Ps, max(NSETS))[1]
    rng = np.random.default_rng(7)
    cots = cotangents(rng, Ps, max(NSETS))
    for n in NSETS:
        (db, dq, dd), dirs = direction_tensors(torch, sv, tile, deltas, n)
        cot, (gux, gpi, glam, gt) = cotangent_tensors(torch, sv, tile, Ps, cots, n)
        t = alternated(torch, dict(tangent=lambda: sv.tangent_sets(db, dq, dd, n),
                                   tangent_dense=lambda: sv.tangent(dirs, n),
                                   adjoint=lambda: sv.adjoint_sets(gux, gpi, glam, gt, n),
                                   adjoint_dense=lambda: sv.adjoint(cot, n)), a.warmup, a.runs)
        nsets = a.nprob * n
        for name, r in t.items():
            nbytes = out["bytes_per_set"]["tangent" if name.startswith("tangent") else "adjoint"]
            r.update(us_per_set=r["ms"] * 1e3 / nsets, GBps=nbytes * nsets / (r["ms"] * 1e-3) / 1e9,
                     spread_us_per_set=(r["ms_max"] - r["ms_min"]) * 1e3 / nsets)
        t["sets"] = nsets
        t["adjoint_over_tangent"] = t["adjoint"]["ms"] / t["tangent"]["ms"]
        t["dense_adjoint_over_tangent"] = t["adjoint_dense"]["ms"] / t["tangent_dense"]["ms"]
        t["excess_us_per_set"] = (t["adjoint"]["ms"] - t["tangent"]["ms"]) * 1e3 / nsets
        t["finite"] = bool(all(torch.isfinite(x).all().item() for x in sv.grad_buffers(n).values()))
        out[f"nsets{n}"] = t
        del db, dq, dd, dirs, cot, gux, gpi, glam, gt
    # the feedback gain both ways, and how far the two results are apart
    nu0, nx1, nx0 = sv.nu[0], sv.nx[1], NX
    A0 = torch.from_numpy(tile(rng.standard_normal((nd, nx1, nx0)))).to(sv.dev)
    S0 = torch.from_numpy(tile(rng.standard_normal((nd, nu0, nx0)))).to(sv.dev)
    g = alternated(torch, dict(gain_tangent=lambda: sv.feedback_gain(A0, S0),
                               gain_adjoint=lambda: sv.feedback_gain_adjoint(A0, S0)), a.warmup, a.runs)
    Kt, Ka = sv.feedback_gain(A0, S0).clone(), sv.feedback_gain_adjoint(A0, S0)
    for r in g.values():
        r.update(us_per_problem=r["ms"] * 1e3 / a.nprob, spread_us_per_problem=(r["ms_max"] - r["ms_min"]) * 1e3 / a.nprob)
    g.update(nx0=nx0, nu0=nu0, tangent_sets=nx0, adjoint_sets=nu0,
             adjoint_over_tangent=g["gain_adjoint"]["ms"] / g["gain_tangent"]["ms"],
             max_abs_difference=float((Kt - Ka).abs().max().item()), max_abs_gain=float(Kt.abs().max().item()))
    out["gain"] = g
    emit(out, a.out)


if __name__ == "__main__":
    main()

"""Time the OCP matrix directions (hpmpc_mi355x_ocp_matrix_dirs_batch / hpmpc_mi355x_ocp_tangent_data_batch,
hk_matdir.hip) beside the dense tangent solve they feed (hpmpc_mi355x_ocp_tangent_batch, hk_tan.hip).

    python tools/kkt_matdir_time.py [--nprob 1024] [--distinct 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: that of tools/batch_time.py and tools/kkt_matgrad_time.py (N = 100, nx = 12, nu = 4, nx[0] = 0; `nprob`
problems, `distinct` different ones tiled to the batch).  One hpmpc_mi355x_ocp_ipm_batch leaves the factor.  Then, for
ndir = 1, 4 direction sets per problem (the vector directions of tools/kkt_tangent_time.py, standard-normal directions
on every element of A, B, Q, S, R, C, D):
  tangent_dense : OcpBatchSolver.tangent, the seven vector directions -- the call as it was before the matrix
                  directions, the yardstick;
  tangent_data  : OcpBatchSolver.tangent_data, all fourteen directions (hk_ocp_matdir, then hk_kkt_tan);
  matdir        : OcpBatchSolver.matrix_directions alone, all fourteen directions, into padded seed rows.
hipEvents around each call; per run the legs are called one after another (alternated in one process, so that clock and
thermal drift hit them alike), `warmup` such rounds, then the median, minimum and maximum of `runs`.  us per set, and
for matdir GB/s against the bytes a set must move: per stage nx1 (nu + nx) + (nu + nx)^2 + ng (nu + nx) direction
doubles, 64 of the base iterate (shared by a problem's sets and counted once per set all the same) and up to 64 of the
vector directions read, 64 written.  Prints one JSON line.
"""
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_time import alternated, direction_tensors, emit, parser, rhs_sets, solved_batch  # noqa: E402

NDIR = (1, 4)


def matdir_bytes(sv):
    """Bytes one set must move through hk_ocp_matdir: every element of the fourteen dense directions and the stage's
    ux, pi, lam slots (64 doubles) read, the stage's seed row (64 doubles) written."""
    from hpmpc_amd.ocp_batch import KEYS

    return 8 * (sum(sv.sizes[key] for key in KEYS) + 128 * (sv.N + 1))


def main():
    a = parser().parse_args()
    import torch

    from hpmpc_amd.ocp_batch import MAT_KEYS, OUT_KEYS

    Ps, nd, sv, tile, out = solved_batch(torch, a, lambda sv: dict(matdir=matdir_bytes(sv)))
    nux = sv.nu[1] + sv.nx[1]  # an inner stage: nx1 (nu + nx) + (nu + nx)^2 + ng (nu + nx)
    out["direction_doubles_per_inner_stage"] = sv.nx[2] * nux + nux * nux + sv.ng[1] * nux
    _, deltas = rhs_sets(Ps, max(NDIR))
    rng = np.random.default_rng(11)
    mats = {key: rng.standard_normal((nd, max(NDIR), sv.sizes[key])) for key in MAT_KEYS}
    for n in NDIR:
        _, vec = direction_tensors(torch, sv, tile, deltas, n)
        dirs = dict(vec, **{key: torch.from_numpy(tile(np.ascontiguousarray(v[:, :n]))).to(sv.dev)
                            for key, v in mats.items()})
        t = alternated(torch, dict(tangent_dense=lambda: sv.tangent(vec, n),
                                   tangent_data=lambda: sv.tangent_data(dirs, n),
                                   matdir=lambda: sv.matrix_directions(dirs, n)), a.warmup, a.runs)
        nsets = a.nprob * n
        for r in t.values():
            r.update(us_per_set=r["ms"] * 1e3 / nsets, spread_us_per_set=(r["ms_max"] - r["ms_min"]) * 1e3 / nsets)
        t["matdir"]["GBps"] = out["bytes_per_set"]["matdir"] * nsets / (t["matdir"]["ms"] * 1e-3) / 1e9
        t["sets"] = nsets
        t["data_over_dense"] = t["tangent_data"]["ms"] / t["tangent_dense"]["ms"]
        t["excess_us_per_set"] = (t["tangent_data"]["ms"] - t["tangent_dense"]["ms"]) * 1e3 / nsets
        got = sv.tangent_data(dirs, n)
        t["finite"] = bool(all(torch.isfinite(got[key]).all().item() for key in OUT_KEYS))
        t["max_abs"] = {key: float(got[key].abs().max().item()) for key in OUT_KEYS if got[key].numel()}
        out[f"ndir{n}"] = t
        del vec, dirs, got
    emit(out, a.out)


if __name__ == "__main__":
    main()

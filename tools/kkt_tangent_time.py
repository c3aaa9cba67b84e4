"""Time the batched KKT tangent solve (hpmpc_mi355x_kkt_tangent_batch / hpmpc_mi355x_ocp_tangent_batch, hk_tan.hip)
beside the re-solve it is the linear part of (hpmpc_mi355x_kkt_new_rhs_batch, hk_kkt.hip), at equal set counts.

    python tools/kkt_tangent_time.py [--nprob 1024] [--distinct 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: that of tools/batch_time.py (`nprob` problems, `distinct` different ones tiled to the batch; every problem and
every set still has its own arrays in HBM).  One hpmpc_mi355x_ocp_ipm_batch leaves the factor.  Then, for ndir = 1, 8,
12 sets per problem:
  resolve : OcpBatchSolver.kkt_sets with explicit b, q, d (IO.new_rhs of each problem), hk_kkt_rhs;
  resolve_dense : the same with dense=True, so with the multi-set finish (hk_ocp_unpack) after it: the finish's cost
            is this leg minus `resolve`;
  tangent : OcpBatchSolver.tangent_sets with the directions new_rhs - problem (padded arrays), hk_kkt_tan;
  dense   : OcpBatchSolver.tangent with the same directions as dense tensors (the same kernel with its dense prologue
            and epilogue).
hipEvents around each call; per run the four are called one after another (alternated in one process, so that clock
and thermal drift hit them alike), `warmup` such rounds, then the median, minimum and maximum of `runs`.  us per set
and GB/s against the bytes a set must move (its problem's BAbt, RSQrq and factor once, its vectors in and out;
work-vector traffic not counted).  Prints one JSON line.
"""
import os
import sys

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_time import alternated, direction_tensors, emit, parser, rhs_sets, set_tensors, solved_batch  # noqa: E402
from kkt_batch_time import set_bytes  # noqa: E402

NDIR = (1, 8, 12)


def tangent_bytes(sv):
    """Bytes one direction must move: BAbt, RSQrq, DCt and the factor records read once, db, dq, dd, t^-1 and the
    multiplier backup read, dux, dpi, dlam, dt written (16- / 32-double stage slots)."""
    n1 = sv.N + 1
    s = sv.sizes
    return 8 * (s["BAbt"] + s["RSQrq"] + s["DCt"] + 352 * n1 + (2 * 16 + 32) * n1 + 2 * 32 * n1 +
                (2 * 16 + 2 * 32) * n1)


def main():
    a = parser().parse_args()
    import torch

    from hpmpc_amd.ocp_batch import kkt_set_arrays

    Ps, nd, sv, tile, out = solved_batch(torch, a, lambda sv: dict(resolve=set_bytes(sv), tangent=tangent_bytes(sv)))
    sets, deltas = rhs_sets(Ps, max(NDIR))
    for ndir in NDIR:
        b, q, d = set_tensors(torch, sv, tile, kkt_set_arrays([S for row in sets for S in row[:ndir]]), ndir)
        (db, dq, dd), dirs = direction_tensors(torch, sv, tile, deltas, ndir)
        t = alternated(torch, dict(resolve=lambda: sv.kkt_sets(b, q, d, nrhs=ndir),
                                   resolve_dense=lambda: sv.kkt_sets(b, q, d, nrhs=ndir, dense=True),
                                   tangent=lambda: sv.tangent_sets(db, dq, dd, ndir),
                                   dense=lambda: sv.tangent(dirs, ndir)), a.warmup, a.runs)
        nsets = a.nprob * ndir
        for name, r in t.items():
            nbytes = out["bytes_per_set"]["resolve" if name.startswith("resolve") else "tangent"]
            r.update(us_per_set=r["ms"] * 1e3 / nsets, GBps=nbytes * nsets / (r["ms"] * 1e-3) / 1e9)
        t["sets"] = nsets
        t["tangent_over_resolve"] = t["tangent"]["ms"] / t["resolve"]["ms"]
        t["dense_over_resolve"] = t["dense"]["ms"] / t["resolve"]["ms"]
        t["unpack_sets_ms"] = t["resolve_dense"]["ms"] - t["resolve"]["ms"]
        # per-set excess of the tangent over the re-solve against the runs' own min-max spread (us per set)
        t["excess_us_per_set"] = (t["tangent"]["ms"] - t["resolve"]["ms"]) * 1e3 / nsets
        t["spread_us_per_set"] = max(r["ms_max"] - r["ms_min"] for r in (t["tangent"], t["resolve"])) * 1e3 / nsets
        t["finite"] = bool(torch.isfinite(sv.set_buffers(ndir)["x"]).all().item())
        out[f"ndir{ndir}"] = t
        del b, q, d, db, dq, dd, dirs
    emit(out, a.out)


if __name__ == "__main__":
    main()

"""Time the batched KKT re-solve (hpmpc_mi355x_kkt_new_rhs_batch, hk_kkt.hip) against a whole batched solve and
against the one-problem entry point that was the only route to a re-solve before it.

    python tools/kkt_batch_time.py [--nprob 1024] [--distinct 64] [--base 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: that of tools/batch_time.py (`nprob` problems, `distinct` different ones tiled to the batch; every problem and
every right-hand-side set still has its own arrays in HBM).
  solve            : hpmpc_mi355x_ocp_ipm_batch on the batch, hipEvents around the call, `warmup` runs, then the
                     median of `runs`; it leaves the factor the re-solves use;
  resolve nrhs=1,8 : OcpBatchSolver.kkt_sets with explicit b, q, d (IO.new_rhs of each problem), timed the same way;
                     us per set and GB/s against the bytes a set must move (its problem's BAbt, RSQrq and factor
                     once, its vectors in and out; work-vector traffic not counted);
  part 1           : wall clock of a loop of d_kkt_solve_new_rhs_res_mpc_hard_tv calls (host buffers, one problem a
                     call) on `base` problems after their own d_ip2_res_mpc_hard_tv, scaled by nprob / base (scaled,
                     not measured on the whole batch).
Prints one JSON line.
"""
import os
import sys
import time

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_time import ARGS, CASE, emit, parser, rhs_sets, set_tensors, tiled_batch, timed  # noqa: E402

NRHS = (1, 8)


def set_bytes(sv):
    """Bytes one right-hand-side set must move: BAbt, RSQrq, DCt and the factor records read once, b, q, d and the
    four backups read, ux, pi, lam, t written (16- / 32-double stage slots)."""
    n1 = sv.N + 1
    s = sv.sizes
    return 8 * (s["BAbt"] + s["RSQrq"] + s["DCt"] + 352 * n1 + (2 * 16 + 32) * n1 + 2 * (2 * 16 + 2 * 32) * n1)


def part1_loop(Ps, sets):
    """d_ip2_res_mpc_hard_tv per problem (untimed), then the timed loop of one-problem re-solves."""
    import iface_oracle as IO
    from hpmpc_amd.batch import LIBPATH
    from hpmpc_amd.cabi import HpmpcAPI, bq_from_qp, load

    api = HpmpcAPI(load(LIBPATH), "")
    work, rhs = [], []
    for P, P2 in zip(Ps, sets):
        work.append(api.ipm(IO.to_qp(P), k_max=50, **ARGS)["work"])
        qp2 = IO.to_qp(P2)
        rhs.append((qp2,) + bq_from_qp(qp2))
    api.kkt_new_rhs(rhs[0][0].copy(), work[0], rhs[0][1], rhs[0][2])  # warm-up
    t0 = time.perf_counter()
    for w, (qp2, b2, q2) in zip(work, rhs):
        api.kkt_new_rhs(qp2, w, b2, q2)
    return (time.perf_counter() - t0) * 1e3


def main():
    a = parser(base=64).parse_args()
    import torch

    from hpmpc_amd.ocp_batch import kkt_set_arrays

    Ps, nd, sv, tile, data = tiled_batch(torch, a.nprob, a.distinct)
    sv.pack(data)
    out = dict(case=CASE, nprob=a.nprob, distinct=nd,
               args=ARGS, runs=a.runs, warmup=a.warmup, bytes_per_set=set_bytes(sv))
    out["solve"] = timed(torch, lambda: sv.solve(**ARGS), a.warmup, a.runs)
    kk, ret = sv.kk.cpu().numpy(), sv.ret.cpu().numpy()
    out["solve"].update(kk_min=int(kk.min()), kk_max=int(kk.max()), kk_sum=int(kk.sum()),
                        ret_nonzero=int((ret != 0).sum()))
    sets = rhs_sets(Ps, max(NRHS))[0]
    for nrhs in NRHS:
        b, q, d = set_tensors(torch, sv, tile, kkt_set_arrays([S for row in sets for S in row[:nrhs]]), nrhs)
        t = timed(torch, lambda: sv.kkt_sets(b, q, d, nrhs=nrhs), a.warmup, a.runs)
        nsets = a.nprob * nrhs
        t.update(sets=nsets, us_per_set=t["ms"] * 1e3 / nsets, GBps=out["bytes_per_set"] * nsets / (t["ms"] * 1e-3) / 1e9,
                 solve_over_resolve=out["solve"]["ms"] / t["ms"])
        ux = sv.kkt_buffers(nrhs)["ux"]
        t["finite"] = bool(torch.isfinite(ux).all().item())
        out[f"resolve_nrhs{nrhs}"] = t
        del b, q, d
    nb = min(a.base, nd)
    ms = part1_loop(Ps[:nb], [row[0] for row in sets[:nb]])
    out["part1_loop"] = dict(problems=nb, ms_measured=ms, scale=a.nprob / nb, ms_scaled=ms * a.nprob / nb,
                             label="scaled from %d problems, not measured on the batch" % nb)
    out["part1_over_resolve_nrhs1"] = out["part1_loop"]["ms_scaled"] / out["resolve_nrhs1"]["ms"]
    emit(out, a.out)


if __name__ == "__main__":
    main()

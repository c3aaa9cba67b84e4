"""Time the batched OCP front end (hpmpc_amd/ocp_batch.py: hk_ocp_pack, the IPM, hk_res + hk_ocp_unpack) against
the host packing route that was the only one before it.

    python tools/ocp_batch_time.py [--nprob 1024] [--distinct 64] [--base 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: that of tools/batch_time.py (`nprob` problems, `distinct` different ones tiled to the batch).
  pack, pack (matrices=0), finish, solve : hipEvents around the call, `warmup` runs, then the median of `runs`;
  TB/s                                   : against the bytes the call must read plus write (algorithmic: every dense
                                           input once, every output element once; for finish the two kernels' inputs
                                           and outputs, hk_res's lib4 blocks included);
  host route                             : wall clock of to_qp per problem + stacking + pack_batch +
                                           torch.from_numpy(..).to(device) for `base` problems, scaled by nprob/base
                                           (scaled, not measured on the whole batch).
Prints one JSON line.
"""
import argparse
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from batch_time import ARGS, CASE, emit, tiled_batch, timed  # noqa: E402


def byte_counts(sv):
    """Bytes per problem each call must read plus write."""
    s = sv.sizes
    dense = sum(s[k] for k in ("A", "B", "b", "Q", "S", "R", "q", "r", "lb", "ub", "C", "D", "lg", "ug"))
    n1 = sv.N + 1
    nux = [sv.nu[k] + sv.nx[k] for k in range(n1)]
    nx1 = [sv.nx[k + 1] if k < sv.N else 0 for k in range(n1)]
    cons = [2 * sv.nb[k] + 2 * sv.ng[k] for k in range(n1)]
    vec_in = sum(s[k] for k in ("b", "q", "r", "lb", "ub", "lg", "ug"))
    pack = dense + s["BAbt"] + s["RSQrq"] + s["DCt"] + s["d"]
    pack_vec = vec_in + sum(nx1) + sum(nux) + s["d"]
    res = s["BAbt"] + s["RSQrq"] + s["DCt"] + sum(nux) + sum(nx1) + 3 * sum(cons) + sum(nux) + sum(nx1) + 2 * sum(cons)
    fin = 2 * sum(nux) + 2 * sum(nx1) + 4 * sum(cons) + sum(nux) + sum(nx1) + 2 * sum(cons) + 4
    return dict(pack=8 * pack, pack_vectors=8 * pack_vec, finish=8 * (res + fin))


def host_route(torch, dev, Ps):
    """The parent commit's only route: numpy packing per problem, stacking, one upload per array."""
    import iface_oracle as IO
    from hpmpc_amd.batch import pack_batch
    from hpmpc_amd.ocp import OCPQP

    t0 = time.perf_counter()
    qps = [IO.to_qp(P) for P in Ps]
    q0 = qps[0]
    qp = OCPQP(q0.N, q0.nx, q0.nu, q0.nb, q0.ng, q0.idxb, [np.stack([q.BAbt[k] for q in qps]) for k in range(q0.N)],
               [np.stack([q.RSQrq[k] for q in qps]) for k in range(q0.N + 1)],
               [np.stack([q.d[k] for q in qps]) for k in range(q0.N + 1)], [], len(qps))
    dev_arrays = [torch.from_numpy(a).to(dev) for a in pack_batch(qp)]
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3, dev_arrays


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1024)
    ap.add_argument("--distinct", type=int, default=64)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    Ps, nd, sv, _, data = tiled_batch(torch, a.nprob, a.distinct)
    nbytes = byte_counts(sv)
    out = dict(case=CASE, nprob=a.nprob, distinct=nd,
               order="C", args=ARGS, runs=a.runs, warmup=a.warmup, bytes_per_problem=nbytes)

    def rate(t, key):
        t["TBps"] = nbytes[key] * a.nprob / (t["ms"] * 1e-3) / 1e12
        return t

    out["pack"] = rate(timed(torch, lambda: sv.pack(data), a.warmup, a.runs), "pack")
    out["pack_vectors"] = rate(timed(torch, lambda: sv.pack(data, matrices=False), a.warmup, a.runs), "pack_vectors")
    out["solve"] = timed(torch, lambda: sv.solve(**ARGS), a.warmup, a.runs)
    kk, ret = sv.kk.cpu().numpy(), sv.ret.cpu().numpy()
    out["solve"].update(kk_min=int(kk.min()), kk_max=int(kk.max()), kk_sum=int(kk.sum()),
                        ret_nonzero=int((ret != 0).sum()))
    out["finish"] = rate(timed(torch, lambda: sv.finish(), a.warmup, a.runs), "finish")
    inf = sv.inf_norm_res.cpu().numpy()
    out["inf_norm_res_max"] = [float(v) for v in inf.max(axis=0)]
    step = out["pack"]["ms"] + out["solve"]["ms"] + out["finish"]["ms"]
    out["step_ms"] = step
    out["pack_finish_share"] = (out["pack"]["ms"] + out["finish"]["ms"]) / step
    loop = out["pack_vectors"]["ms"] + out["solve"]["ms"] + out["finish"]["ms"]
    out["pack_vectors_finish_share"] = (out["pack_vectors"]["ms"] + out["finish"]["ms"]) / loop

    nb = min(a.base, nd)
    host_route(torch, sv.dev, Ps[:2])  # warm-up (allocator, first copy)
    ms, arrays = host_route(torch, sv.dev, Ps[:nb])
    same = bool(np.array_equal(arrays[0].cpu().numpy(), sv.BAbt[:nb].cpu().numpy()) and
                np.array_equal(arrays[1].cpu().numpy(), sv.RSQrq[:nb].cpu().numpy()))
    out["host_route"] = dict(problems=nb, ms_measured=ms, scale=a.nprob / nb, ms_scaled=ms * a.nprob / nb,
                             label="scaled from %d problems, not measured on the batch" % nb,
                             same_arrays_as_hk_ocp_pack=same)
    out["host_route_over_pack"] = out["host_route"]["ms_scaled"] / out["pack"]["ms"]
    emit(out, a.out)


if __name__ == "__main__":
    main()

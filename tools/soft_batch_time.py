"""Time the batched soft-constraint IPM (hpmpc_mi355x_ipm_soft_batch) against the loop of single-problem calls.

    python tools/soft_batch_time.py [--nprob 1024] [--base 64] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: `nprob` copies of mass_spring_soft(N=30, nx=8, nu=2) with x0[0] = x0[1] spread over [0.2, 3.5]; k_max 50,
mu0 100, mu_tol 1e-5, alpha_min 1e-8 (the ms_N30_nx8_nu2 case of tests/test_gpu_soft.py).
  batched  : hipEvents around the call (its init launch and its one solve launch), `warmup` runs, then the median
             of `runs`;
  baseline : d_ip2_mpc_soft_tv in a loop over `base` of the problems (every nprob/base-th), wall clock around the
             pre-marshalled foreign calls, one warm-up pass, scaled by nprob/base to the batch.
Prints one JSON line with both times, their ratio, and the IP iterations per second of the batched path.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

ARGS = dict(k_max=50, mu0=100.0, mu_tol=1e-5, alpha_min=1e-8)


def problems(nprob):
    from hpmpc_amd.soft import mass_spring_soft

    out = []
    for s in np.linspace(0.2, 3.5, nprob):
        x0 = np.zeros(8)
        x0[0] = x0[1] = s
        out.append(mass_spring_soft(N=30, nx=8, nu=2, x0=x0))
    return out


def single_call(api, sq):
    """A pre-marshalled d_ip2_mpc_soft_tv call on private buffers: returns (call, kk)."""
    from hpmpc_amd.cabi import ipp, iv

    N, k_max = sq.N, ARGS["k_max"]
    ux, pi, lam, t = sq.alloc_solution()
    stat, work, kk = np.zeros(5 * k_max + 5), np.zeros(64), C.c_int(0)
    dct = [np.zeros(8)] * (N + 1)
    keep = (ux, pi, lam, t, stat, work, dct, sq)
    args = (C.byref(kk), C.c_int(k_max), C.c_double(ARGS["mu0"]), C.c_double(ARGS["mu_tol"]),
            C.c_double(ARGS["alpha_min"]), C.c_int(0), api._p(stat), C.c_int(N), iv(sq.nx), iv(sq.nu), iv(sq.nb),
            ipp(sq.idxb), iv(sq.ng), iv(sq.ns), api._pp(sq.BAbt), api._pp(sq.RSQrq), api._pp(sq.Z), api._pp(sq.z),
            api._pp(dct), api._pp(sq.d), api._pp(ux), C.c_int(1), api._pp(pi), api._pp(lam), api._pp(t), api._p(work))
    fn = api.fn("d_ip2_mpc_soft_tv")

    def call(_keep=keep):
        return fn(*args)

    return call, kk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1024)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    from hpmpc_amd.batch import LIBPATH
    from hpmpc_amd.cabi import HpmpcAPI, load
    from hpmpc_amd.soft import SoftBatchSolver

    sqs = problems(a.nprob)
    sv = SoftBatchSolver(sqs, k_max=ARGS["k_max"])
    ms = []
    for i in range(a.warmup + a.runs):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        sv.solve(**ARGS)
        e1.record()
        torch.cuda.synchronize()
        if i >= a.warmup:
            ms.append(e0.elapsed_time(e1))
    kk = sv.kk.cpu().numpy()
    ret = sv.ret.cpu().numpy()
    batched_ms = float(np.median(ms))

    api = HpmpcAPI(load(LIBPATH), "")
    step = max(1, a.nprob // a.base)
    sub = list(range(0, a.nprob, step))[:a.base]
    calls = [single_call(api, sqs[p]) for p in sub]
    for call, _ in calls:  # warm-up pass (plan cache, arenas)
        call()
    t0 = time.perf_counter()
    rets = [call() for call, _ in calls]
    loop_ms = (time.perf_counter() - t0) * 1e3
    scale = a.nprob / len(sub)
    same = all(int(k.value) == int(kk[p]) and int(r) == int(ret[p]) for (c, k), r, p in zip(calls, rets, sub))
    res = dict(case="mass_spring_soft N=30 nx=8 nu=2", nprob=a.nprob, args=ARGS, batched_ms=batched_ms,
               batched_ms_min=float(min(ms)), batched_ms_max=float(max(ms)), runs=a.runs, warmup=a.warmup,
               kk_min=int(kk.min()), kk_max=int(kk.max()), kk_sum=int(kk.sum()), ret_nonzero=int((ret != 0).sum()),
               ip_iters_per_s=float(kk.sum() / (batched_ms * 1e-3)), batched_us_per_problem=batched_ms * 1e3 / a.nprob,
               loop_problems=len(sub), loop_ms_measured=loop_ms, loop_scale=scale, loop_ms_scaled=loop_ms * scale,
               loop_us_per_problem=loop_ms * 1e3 / len(sub), speedup=loop_ms * scale / batched_ms,
               kk_ret_same_as_loop=bool(same))
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

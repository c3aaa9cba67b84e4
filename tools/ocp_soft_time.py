"""Time the soft OCP front end (hpmpc_mi355x_ocp_soft_*: pack + solve + finish on dense device data) against the loop
of one-problem fortran_order_d_ip_ocp_soft_tv calls.

    python tools/ocp_soft_time.py [--nprob 1024] [--base 64] [--N 30] [--nx 8] [--nu 3] [--warmup 3] [--runs 10]
                                  [--out FILE.json]

Batch: `nprob` draws of oracle/iface_oracle.py random_soft_iface_problem(N, nx, nu) -- the reference driver's shape:
hard boxes on every input, soft boxes on every state, x0 folded into stage 0 -- seeds 0 .. nprob-1; k_max 50, mu0 100,
mu_tol 1e-6.  No z is given, as the one-problem wrapper uses none.
  batched  : hipEvents around pack(), solve() and finish() with the residual norms (six launches, no host copy),
             `warmup` runs, then the median of `runs`; the dense data are on the device before the clock starts;
  vectors  : the same with pack(matrices=False), the receding-horizon step;
  baseline : fortran_order_d_ip_ocp_soft_tv in a loop over `base` of the problems (every nprob/base-th), wall clock
             around the pre-marshalled foreign calls, one warm-up pass, scaled by nprob/base to the batch.
Prints one JSON line with the times, their ratio, and whether kk / status of the looped problems equal the batch's.
"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ARGS = dict(k_max=50, mu0=100.0, mu_tol=1e-6)


def single_call(api, P):
    """A pre-marshalled fortran_order_d_ip_ocp_soft_tv call on private buffers: returns (call, kk, inf_norm_res)."""
    from hpmpc_amd.cabi import _dptr, dpp, ipp, iv

    N, k_max = P["N"], ARGS["k_max"]
    nx, nu, nb, ng, ns = iv(P["nx"]), iv(P["nu"]), iv(P["nb"]), iv(P["ng"]), iv(P["ns"])
    idx = [np.ascontiguousarray(i, dtype=np.int32) for i in P["hidxb"]]
    a = api._iface_args(P, "F")
    pad = lambda v: np.concatenate([np.asarray(v, dtype=np.float64), np.zeros(4)])
    Z, z = [pad(v) for v in P["Z"]], [pad(v) for v in P["z"]]
    x = [np.zeros(P["nx"][k] + 4) for k in range(N + 1)]
    u = [np.zeros(P["nu"][k] + 4) for k in range(N + 1)]
    pi = [np.zeros(P["nx"][k + 1] + 4) for k in range(N)]
    lam = [np.zeros(2 * P["nb"][k] + 4 * P["ns"][k] + 4) for k in range(N + 1)]
    inf, stat, kk = np.zeros(4), np.zeros(5 * k_max + 5), C.c_int(0)
    wsz = api.fn("hpmpc_d_ip_ocp_soft_tv_work_space_size_bytes")(C.c_int(N), nx, nu, nb, ipp(idx), ng, ns)
    work0 = np.zeros(wsz // 8 + 16)
    keep = (nx, nu, nb, ng, ns, idx, a, Z, z, x, u, pi, lam, inf, stat, work0)
    args = (C.byref(kk), C.c_int(k_max), C.c_double(ARGS["mu0"]), C.c_double(ARGS["mu_tol"]), C.c_int(N), nx, nu, nb,
            ipp(idx), ng, ns, C.c_int(0), dpp(a["A"]), dpp(a["B"]), dpp(a["b"]), dpp(a["Q"]), dpp(a["S"]), dpp(a["R"]),
            dpp(a["q"]), dpp(a["r"]), dpp(Z), dpp(z), dpp(a["lb"]), dpp(a["ub"]), dpp(a["C"]), dpp(a["D"]),
            dpp(a["lg"]), dpp(a["ug"]), dpp(x), dpp(u), dpp(pi), dpp(lam), _dptr(inf), _dptr(work0), _dptr(stat))
    fn = api.fn("fortran_order_d_ip_ocp_soft_tv")

    def call(_keep=keep):
        return fn(*args)

    return call, kk, inf


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1024)
    ap.add_argument("--base", type=int, default=64)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--nx", type=int, default=8)
    ap.add_argument("--nu", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import iface_oracle as IO
    from hpmpc_amd.batch import LIBPATH
    from hpmpc_amd.cabi import HpmpcAPI, load
    from hpmpc_amd.ocp_soft import OcpSoftBatchSolver, flatten_soft_problems

    Ps = [IO.random_soft_iface_problem(a.N, a.nx, a.nu, seed=s) for s in range(a.nprob)]
    flat = flatten_soft_problems(Ps, "F")
    del flat["z"]
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for k, v in flat.items()}
    P = Ps[0]
    sv = OcpSoftBatchSolver(P["N"], P["nx"], P["nu"], P["nb"], P["hidxb"], P["ns"], data, nprob=a.nprob, order="F",
                            k_max=ARGS["k_max"])
    assert sv.res_ok

    def timed(matrices):
        """Per run (total, pack, solve, finish) in ms, from four events on the stream."""
        ms = []
        for i in range(a.warmup + a.runs):
            ev = [torch.cuda.Event(enable_timing=True) for _ in range(4)]
            ev[0].record()
            sv.pack(matrices=matrices)
            ev[1].record()
            sv.solve(mu0=ARGS["mu0"], mu_tol=ARGS["mu_tol"])
            ev[2].record()
            sv.finish(norms=True)
            ev[3].record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append([ev[0].elapsed_time(ev[3])] + [ev[j].elapsed_time(ev[j + 1]) for j in range(3)])
        return np.array(ms)

    full, vec = timed(True), timed(False)
    phases = {k: float(np.median(full[:, j + 1])) for j, k in enumerate(("pack_ms", "solve_ms", "finish_ms"))}
    phases["pack_vectors_only_ms"] = float(np.median(vec[:, 1]))
    full, vec = full[:, 0], vec[:, 0]
    kk, ret = sv.kk.cpu().numpy(), sv.ret.cpu().numpy()
    inf = sv.inf_norm_res.cpu().numpy()
    batched_ms = float(np.median(full))

    api = HpmpcAPI(load(LIBPATH), "")
    step = max(1, a.nprob // a.base)
    sub = list(range(0, a.nprob, step))[:a.base]
    calls = [single_call(api, Ps[p]) for p in sub]
    for call, _, _ in calls:  # warm-up pass (plan cache, arenas)
        call()
    t0 = time.perf_counter()
    rets = [call() for call, _, _ in calls]
    loop_ms = (time.perf_counter() - t0) * 1e3
    scale = a.nprob / len(sub)
    same = all(int(k.value) == int(kk[p]) and int(r) == int(ret[p]) for (c, k, _), r, p in zip(calls, rets, sub))
    inf_diff = max(float(np.max(np.abs(i - inf[p]))) for (_, _, i), p in zip(calls, sub))
    res = dict(case=f"random_soft_iface_problem N={a.N} nx={a.nx} nu={a.nu}", nprob=a.nprob, args=ARGS,
               batched_ms=batched_ms, batched_ms_min=float(min(full)), batched_ms_max=float(max(full)),
               vectors_only_ms=float(np.median(vec)), **phases, runs=a.runs, warmup=a.warmup, kk_min=int(kk.min()),
               kk_max=int(kk.max()), kk_sum=int(kk.sum()), ret_nonzero=int((ret != 0).sum()),
               batched_us_per_problem=batched_ms * 1e3 / a.nprob, loop_problems=len(sub), loop_ms_measured=loop_ms,
               loop_scale=scale, loop_ms_scaled=loop_ms * scale, loop_us_per_problem=loop_ms * 1e3 / len(sub),
               speedup=loop_ms * scale / batched_ms, kk_status_same_as_loop=bool(same),
               inf_norm_res_max_abs_diff_to_loop=inf_diff)
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

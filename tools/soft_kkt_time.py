"""Time the batched soft KKT re-solve (hpmpc_mi355x_soft_kkt_ocp_batch / hpmpc_mi355x_soft_kkt_batch) beside the full
receding-horizon step of the soft OCP front end on the same batch.

    python tools/soft_kkt_time.py [--nprob 1024] [--N 30] [--nx 8] [--nu 3] [--warmup 3] [--runs 10] [--out FILE.json]

Batch: `nprob` draws of oracle/iface_oracle.py random_soft_iface_problem(N, nx, nu), seeds 0 .. nprob-1, as
tools/ocp_soft_time.py; k_max 50, mu0 100, mu_tol 1e-6, no z.  The sets are the problems' own b, q, r, lb, ub with
0.05 N(0,1) added to b, q, r and the bounds widened by 0.05 |N(0,1)|, drawn on the device.
  step     : hipEvents around pack(matrices=False) + solve() + finish() with the residual norms;
  kkt_sets : hipEvents around OcpSoftBatchSolver.kkt_sets at nrhs 1 and 8, refactor 0 (the linearisation the solve
             left) and 1 (at the returned iterate): pack, [factor,] sets, unpack;
  core     : hpmpc_mi355x_soft_kkt_batch alone on the packed per-set vectors of that call, refactor 0 (the set launch)
             and 1 (factor launch + set launch); their difference is the factor launch, kkt_sets - core the pack and
             unpack launches.
`warmup` runs, then the median of `runs`.  Prints one JSON line: the times, the time per set and its ratio to the step.
"""
import argparse
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

ARGS = dict(k_max=50, mu0=100.0, mu_tol=1e-6)
SET_KEYS = ("b", "q", "r", "lb", "ub")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--nprob", type=int, default=1024)
    ap.add_argument("--N", type=int, default=30)
    ap.add_argument("--nx", type=int, default=8)
    ap.add_argument("--nu", type=int, default=3)
    ap.add_argument("--warmup", type=int, default=3)
    ap.add_argument("--runs", type=int, default=10)
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    import torch

    import iface_oracle as IO
    from hpmpc_amd.bindings import check, lib
    from hpmpc_amd.ocp_soft import OcpSoftBatchSolver, flatten_soft_problems

    Ps = [IO.random_soft_iface_problem(a.N, a.nx, a.nu, seed=s) for s in range(a.nprob)]
    flat = flatten_soft_problems(Ps, "F")
    del flat["z"]
    data = {k: torch.from_numpy(np.ascontiguousarray(v)).to("cuda") for k, v in flat.items()}
    P = Ps[0]
    sv = OcpSoftBatchSolver(P["N"], P["nx"], P["nu"], P["nb"], P["hidxb"], P["ns"], data, nprob=a.nprob, order="F",
                            k_max=ARGS["k_max"])
    L = lib()

    def median_ms(fn):
        ms = []
        for i in range(a.warmup + a.runs):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= a.warmup:
                ms.append(e0.elapsed_time(e1))
        return float(np.median(ms))

    def step():
        sv.pack(matrices=False)
        sv.solve(mu0=ARGS["mu0"], mu_tol=ARGS["mu_tol"])
        sv.finish(norms=True)

    sv.pack()
    step_ms = median_ms(step)
    kk = sv.kk.cpu().numpy()
    res = dict(case=f"random_soft_iface_problem N={a.N} nx={a.nx} nu={a.nu}", nprob=a.nprob, args=ARGS, runs=a.runs,
               warmup=a.warmup, step_ms=step_ms, kk_min=int(kk.min()), kk_max=int(kk.max()), kk_sum=int(kk.sum()),
               ret_nonzero=int((sv.ret.cpu().numpy() != 0).sum()), sets={})
    gen = torch.Generator(device="cuda").manual_seed(0)
    n16, sD = (a.N + 1) * 16, sv.sizes["d"]
    soft_plan = L.hpmpc_mi355x_ocp_soft_ipm_plan(sv.plan)
    for nrhs in (1, 8):
        sets = {}
        for key in SET_KEYS:
            base = data[key][:, None, :].expand(-1, nrhs, -1)
            noise = 0.05 * torch.randn(base.shape, generator=gen, device="cuda", dtype=torch.float64)
            sets[key] = (base + noise if key in ("b", "q", "r") else
                         base - noise.abs() if key == "lb" else base + noise.abs()).contiguous()
        o = sv.kkt_buffers(nrhs)
        row = {}
        for refactor in (0, 1):
            row[f"kkt_sets_refactor{refactor}_ms"] = median_ms(lambda: sv.kkt_sets(sets, nrhs, refactor=bool(refactor)))
        # the packed per-set vectors that call left in its work buffer, as arrays of their own for the core call
        w = o["work"]
        b, q = (w[..., i * n16:(i + 1) * n16].contiguous() for i in (0, 1))
        d = w[..., 4 * n16:4 * n16 + sD].contiguous()
        out = [torch.zeros((a.nprob, nrhs, n), dtype=torch.float64, device="cuda")
               for n in (n16, n16, sv.sizes["lam"], sv.sizes["lam"])]

        def core(refactor):
            check(L.hpmpc_mi355x_soft_kkt_batch(
                soft_plan, None, a.nprob, 0, a.nprob, nrhs, sv.BAbt.data_ptr(), sv.RSQrq.data_ptr(), sv.Zp.data_ptr(),
                sv.zp.data_ptr(), sv.lam.data_ptr(), sv.t.data_ptr(), b.data_ptr(), q.data_ptr(), d.data_ptr(), None,
                *[x.data_ptr() for x in out], sv.ws.data_ptr(), o["scratch"].data_ptr(), refactor, 1,
                sv._stream()), "hpmpc_mi355x_soft_kkt_batch")

        for refactor in (0, 1):
            row[f"core_refactor{refactor}_ms"] = median_ms(lambda: core(refactor))
        row["set_launch_ms"] = row["core_refactor0_ms"]
        row["factor_launch_ms"] = row["core_refactor1_ms"] - row["core_refactor0_ms"]
        row["pack_unpack_ms"] = row["kkt_sets_refactor0_ms"] - row["core_refactor0_ms"]
        for refactor in (0, 1):
            t = row[f"kkt_sets_refactor{refactor}_ms"]
            row[f"us_per_set_refactor{refactor}"] = t * 1e3 / (a.nprob * nrhs)
            row[f"share_of_step_per_set_refactor{refactor}"] = t / nrhs / step_ms
        res["sets"][str(nrhs)] = row
    line = json.dumps(res)
    print(line)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write(line + "\n")


if __name__ == "__main__":
    main()

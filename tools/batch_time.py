"""What tools/ocp_batch_time.py, kkt_batch_time.py, kkt_tangent_time.py and kkt_adjoint_time.py share: the batch they time, the event
timers and the one-JSON-line output.

Batch: `nprob` problems of N=100, nx=12, nu=4 (nx[0] = 0) with 4 input and 6 state boxes per stage, from
oracle/iface_oracle.py random_iface_problem; `distinct` different problems are generated and tiled to the batch (every
problem still has its own copy of every array in HBM, so the bytes moved are those of `nprob` different problems).
"""
import json
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "oracle"))

N, NX, NU, NBU, NBX = 100, 12, 4, 4, 6
ARGS = dict(mu0=2.0, mu_tol=1e-10, alpha_min=1e-8)
CASE = f"random_iface_problem N={N} nx={NX} nu={NU} boxes {NBU}+{NBX}"


def alternated(torch, fns, warmup, runs):
    """{name: timing}: each round calls every function once, in order, with its own pair of events; `warmup` rounds,
    then the median, minimum and maximum of `runs`."""
    ms = {name: [] for name in fns}
    for i in range(warmup + runs):
        for name, fn in fns.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            if i >= warmup:
                ms[name].append(e0.elapsed_time(e1))
    return {name: dict(ms=float(np.median(v)), ms_min=float(min(v)), ms_max=float(max(v))) for name, v in ms.items()}


def timed(torch, fn, warmup, runs):
    return alternated(torch, {"fn": fn}, warmup, runs)["fn"]


def tiled_batch(torch, nprob, distinct):
    """(Ps, nd, sv, tile, data): the nd = min(distinct, nprob) generated problems, an OcpBatchSolver for `nprob` of
    them (order "C", k_max 50), tile(array with leading dimension nd) -> the batch's leading dimension nprob, and the
    batch's dense device tensors (not packed yet)."""
    import iface_oracle as IO
    from hpmpc_amd.ocp_batch import OcpBatchSolver, flatten_problems

    nd = min(distinct, nprob)
    Ps = [IO.random_iface_problem(N, [0] + [NX] * N, [NU] * N, NBU, NBX, None, seed=1000 + s) for s in range(nd)]
    P0 = Ps[0]
    sv = OcpBatchSolver(N, P0["nx"], P0["nu"], P0["nb"], P0["hidxb"], P0["ng"], nprob, order="C", k_max=50)
    reps = -(-nprob // nd)
    tile = lambda v: np.tile(v, (reps,) + (1,) * (v.ndim - 1))[:nprob].copy()
    data = {k: torch.from_numpy(tile(v)).to(sv.dev) for k, v in flatten_problems(Ps, "C").items()}
    return Ps, nd, sv, tile, data


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")

"""What tools/ocp_batch_time.py and the kkt_*_time.py tools share: the arguments, the batch they time, its solve, the
direction and cotangent sets, the event timers and the one-JSON-line output.

Batch: `nprob` problems of N=100, nx=12, nu=4 (nx[0] = 0) with 4 input and 6 state boxes per stage, from
oracle/iface_oracle.py random_iface_problem; `distinct` different problems are generated and tiled to the batch (every
problem still has its own copy of every array in HBM, so the bytes moved are those of `nprob` different problems).
"""
import argparse
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


def parser(**extra):
    """--nprob 1024 --distinct 64 [``extra``: further integer options and their defaults] --warmup 3 --runs 10 --out."""
    ap = argparse.ArgumentParser()
    for name, default in dict(nprob=1024, distinct=64, **extra, warmup=3, runs=10).items():
        ap.add_argument("--" + name, type=int, default=default)
    ap.add_argument("--out", default=None)
    return ap


def solved_batch(torch, a, bytes_per_set):
    """(Ps, nd, sv, tile, out): tiled_batch for the arguments ``a``, packed and solved once (the factor the set calls
    use), and the head of the tool's JSON with bytes_per_set(sv) and the solve's iteration counts."""
    Ps, nd, sv, tile, data = tiled_batch(torch, a.nprob, a.distinct)
    sv.pack(data)
    sv.solve(**ARGS)
    torch.cuda.synchronize()
    kk, ret = sv.kk.cpu().numpy(), sv.ret.cpu().numpy()
    out = dict(case=CASE, nprob=a.nprob, distinct=nd, args=ARGS, runs=a.runs, warmup=a.warmup,
               bytes_per_set=bytes_per_set(sv),
               solve=dict(kk_min=int(kk.min()), kk_max=int(kk.max()), ret_nonzero=int((ret != 0).sum())))
    return Ps, nd, sv, tile, out


def rhs_sets(Ps, nmax):
    """(sets, deltas): sets[p][r] = IO.new_rhs(Ps[p], seed=6 + r) for r < nmax, and deltas[p][r] = that set's b, q, r
    and bounds minus the problem's own (interface-form dicts with the sizes)."""
    import iface_oracle as IO
    from hpmpc_amd.ocp_batch import VEC_KEYS

    sets = [[IO.new_rhs(P, seed=6 + r) for r in range(nmax)] for P in Ps]
    sizes = {k: Ps[0][k] for k in ("N", "nx", "nu", "nb", "ng")}
    deltas = [[dict(sizes, **{key: [np.asarray(y) - np.asarray(x) for x, y in zip(P[key], S[key])] for key in VEC_KEYS})
               for S in row] for P, row in zip(Ps, sets)]
    return sets, deltas


def set_tensors(torch, sv, tile, arrays, n):
    """Problem-major per-set host arrays (nd * n, ...) -> device tensors (nprob, n, ...), tiled to the batch."""
    return tuple(torch.from_numpy(tile(x.reshape((-1, n) + x.shape[1:]))).to(sv.dev) for x in arrays)


def direction_tensors(torch, sv, tile, deltas, n):
    """The first n directions per problem of ``deltas``: (db, dq, dd) padded (tangent_sets), and the dense dict
    (tangent)."""
    from hpmpc_amd.ocp_batch import VEC_KEYS, flatten_sets, tangent_set_arrays

    padded = set_tensors(torch, sv, tile, tangent_set_arrays([D for row in deltas for D in row[:n]]), n)
    dirs = {key: torch.from_numpy(tile(v)).to(sv.dev) for key, v in flatten_sets(deltas, n, VEC_KEYS).items()}
    return padded, dirs


def cotangents(rng, Ps, nmax):
    """Standard-normal cotangents on every element of u, x, pi, lam, t: {key: (nd, nmax, size)}."""
    from hpmpc_amd.ocp_batch import OUT_KEYS, ocp_dense_layout

    P0 = Ps[0]
    osz = ocp_dense_layout(P0["N"], P0["nx"], P0["nu"], P0["nb"], P0["ng"])["sizes"]
    return {key: rng.standard_normal((len(Ps), nmax, osz[key])) for key in OUT_KEYS}


def cotangent_tensors(torch, sv, tile, Ps, cots, n):
    """The first n cotangent sets per problem of ``cots``: the dense dict (adjoint, adjoint_data), and (gux, gpi, glam,
    gt) padded (adjoint_sets)."""
    from hpmpc_amd.ocp_batch import OUT_KEYS, adjoint_set_arrays, unflatten_problems

    P0 = Ps[0]
    sizes = {k: P0[k] for k in ("N", "nx", "nu", "nb", "ng")}
    cot = {key: torch.from_numpy(tile(np.ascontiguousarray(v[:, :n]))).to(sv.dev) for key, v in cots.items()}
    per = unflatten_problems({key: v[:, :n].reshape(len(Ps) * n, -1) for key, v in cots.items()}, P0["N"], P0["nx"],
                             P0["nu"], P0["nb"], P0["ng"], keys=list(OUT_KEYS))
    return cot, set_tensors(torch, sv, tile, adjoint_set_arrays([dict(sizes, **G) for G in per]), n)


def emit(out, path):
    line = json.dumps(out)
    print(line)
    if path:
        os.makedirs(os.path.dirname(os.path.abspath(path)), exist_ok=True)
        with open(path, "w") as f:
            f.write(line + "\n")

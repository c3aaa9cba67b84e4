"""bench.py's command line: a plain run measures the headline only, --full adds the other legs, --dump-outputs
writes the last step's converged entries.  The dump is checked on the CPU against a stand-in queue; one small plain
run goes through the GPU."""
import json
import os
import subprocess
import sys
import types

import numpy as np
import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
MOVED = ("k40", "queue_batch_slots", "generic_shape", "isolated_batch", "aliased", "coupled", "riccati", "cpu_baseline",
         "scatter", "pcond", "riccati_batch_N50", "single_qp", "parity")


def _bench():
    sys.path.insert(0, ROOT)
    import bench

    return bench


def test_plain_run_switches_every_other_leg_off(monkeypatch):
    bench = _bench()
    monkeypatch.setattr(sys, "argv", ["bench.py", "--gpus", "1", "--steps", "3", "--warmup", "1"])
    a = bench.parse()
    assert not a.full and a.dump_outputs is None and a.steps == 3
    assert all((a.no_k40, a.no_cpu, a.no_pcond, a.no_isolated, a.no_scatter, a.no_queue_batch_slots, a.no_aliased,
                a.no_coupled))
    monkeypatch.setattr(sys, "argv", ["bench.py", "--full", "--no-cpu", "--dump-outputs", "d"])
    a = bench.parse()
    assert a.full and a.no_cpu and a.dump_outputs == "d"
    assert not any((a.no_k40, a.no_pcond, a.no_isolated, a.no_scatter, a.no_queue_batch_slots, a.no_aliased,
                    a.no_coupled))


def _fake_queue(qp, steps, seed):
    import torch

    g = torch.Generator().manual_seed(seed)
    nq = steps * qp.batch
    q = types.SimpleNamespace()
    for n, w in (("ux", 16), ("pi", 16), ("lam", 32), ("t", 32)):
        setattr(q, n, torch.rand((nq, qp.N + 1, w), dtype=torch.float64, generator=g) + 1.0)  # no zero anywhere
    q.kk = torch.randint(5, 15, (nq,), dtype=torch.int32, generator=g)
    q.ret = (torch.arange(nq) % 5 == 3).to(torch.int32) * 2  # every fifth entry stopped on alpha_min
    return q


def test_dump_outputs_rows_masks_and_budget(tmp_path, monkeypatch):
    from hpmpc_amd.ocp import mass_spring_qp

    bench = _bench()
    B, N, steps = 7, 6, 3
    qp = mass_spring_qp(N, 4, 2, batch=B, time_variant=True, seed=1)
    Q = _fake_queue(qp, steps, 0)
    bench.dump_outputs(str(tmp_path / "a"), qp, Q, steps)
    d = {f[:-4]: np.load(tmp_path / "a" / f) for f in sorted(os.listdir(tmp_path / "a"))}
    assert sorted(d) == ["entries", "kk", "lam", "pi", "ret", "ret_batch", "t", "ux"]
    assert all(v.dtype == np.float64 for v in d.values())
    ret = Q.ret.numpy()
    want = np.array([q for q in range((steps - 1) * B, steps * B) if ret[q] == 0])
    assert np.array_equal(d["entries"], want) and 0 < len(want) < B
    assert np.array_equal(d["ret_batch"], ret[(steps - 1) * B:]) and not d["ret"].any()
    assert np.array_equal(d["kk"], Q.kk.numpy()[want])
    for k in range(N + 1):
        nux, nb, pnb = qp.nux(k), int(qp.nb[k]), qp.pnb(k)
        npi = int(qp.nx[k + 1]) if k < N else 0
        assert np.array_equal(d["ux"][:, k, :nux], Q.ux.numpy()[want, k, :nux]) and not d["ux"][:, k, nux:].any()
        assert np.array_equal(d["pi"][:, k, :npi], Q.pi.numpy()[want, k, :npi]) and not d["pi"][:, k, npi:].any()
        for n in ("lam", "t"):
            src = getattr(Q, n).numpy()[want, k]
            assert np.array_equal(d[n][:, k, :nb], src[:, :nb])
            assert np.array_equal(d[n][:, k, pnb:pnb + nb], src[:, pnb:pnb + nb])
            assert not d[n][:, k, nb:pnb].any() and not d[n][:, k, pnb + nb:].any()
    # over the byte budget: a fixed sample of the batch, the same on every call
    per_entry = 8 * ((N + 1) * 96 + 3)
    monkeypatch.setattr(bench, "DUMP_MAX_BYTES", 4 * per_entry)
    for name in ("b", "c"):
        bench.dump_outputs(str(tmp_path / name), qp, Q, steps)
    e = np.load(tmp_path / "b" / "entries.npy")
    assert np.array_equal(e, np.load(tmp_path / "c" / "entries.npy"))
    assert len(e) <= 4 and set(e) <= set(want) and np.all(np.diff(e) > 0)
    assert sum(os.path.getsize(tmp_path / "b" / f) for f in os.listdir(tmp_path / "b")) <= 4 * per_entry + 8 * 128 + 8 * B


@pytest.mark.gpu
def test_plain_run_line_and_dump(tmp_path):
    """One small plain run: the headline's fields are there, the other legs' are null, --steps sets the timed steps
    (every entry of steps x batch solved: sum_kk_per_step x steps = value x ms_per_step x steps), the dump loads."""
    steps, B = 3, 64
    r = subprocess.run([sys.executable, os.path.join(ROOT, "bench.py"), "--gpus", "1", "--steps", str(steps), "--warmup",
                        "1", "--batch", str(B), "--N", "10", "--dump-outputs", str(tmp_path / "out")],
                       capture_output=True, text=True, timeout=120, cwd=str(tmp_path))
    assert r.returncode == 0, r.stderr[-2000:]
    lines = [x for x in r.stdout.splitlines() if x.startswith("{")]
    assert len(lines) == 1
    d = json.loads(lines[0])
    assert d["unit"] == "IP-iter/s" and d["higher_is_better"] is True and d["dtype"] == "f64" and d["steps"] == steps
    assert d["metric"].startswith("Riccati factorisations/sec + IP iters/sec")
    assert d["value"] > 0 and d["ms_per_step"] > 0
    assert all(d[k] is None for k in MOVED)
    iters = d["config"]["sum_kk_per_step"] * steps
    assert iters >= steps * B  # every entry of every step took at least one iteration
    assert abs(d["value"] * d["ms_per_step"] * 1e-3 * steps - iters) <= 1e-9 * iters
    out = {f[:-4]: np.load(tmp_path / "out" / f) for f in os.listdir(tmp_path / "out")}
    assert sorted(out) == ["entries", "kk", "lam", "pi", "ret", "ret_batch", "t", "ux"]
    n = len(out["entries"])
    assert 0 < n <= B and out["ret_batch"].shape == (B,) and n == int((out["ret_batch"] == 0).sum())
    assert out["entries"].min() >= (steps - 1) * B and out["entries"].max() < steps * B
    assert out["ux"].shape == (n, 11, 16) and out["lam"].shape == (n, 11, 32)
    assert all(np.isfinite(v).all() for v in out.values()) and np.abs(out["ux"]).max() > 0

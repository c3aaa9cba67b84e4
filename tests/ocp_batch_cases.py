"""Shared by tests/test_gpu_ocp_batch.py and tests/test_gpu_ocp_batch_general.py: the cases of the batched OCP front
end, the expected lib4 arrays from oracle/iface_oracle.py to_qp, and the gates of tests/test_gpu_iface.py."""
import os
import sys

import numpy as np

from helpers import TOL_IPM

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import iface_oracle as IO  # noqa: E402

# N, nx, nu, boxed inputs, boxed states, ng
CASES = {
    # odd sizes, several panels, an empty x_0, general constraints on inner stages and on stage N
    "V": (5, [0, 3, 3, 5, 5, 4], [2, 2, 1, 3, 3], 2, 2, [0, 0, 2, 0, 3, 2]),
    "V0": (5, [0, 3, 3, 5, 5, 4], [2, 2, 1, 3, 3], 2, 2, None),  # the same without general constraints
    "F": (4, [0, 8, 8, 8, 8], [3, 3, 3, 3], 3, 4, None),         # inner stages of the compiled (3, 8) class
    "S": (1, [2, 2], [1], 1, 1, None),                           # smallest horizon
    "R": (2, [2, 2, 2], [1, 1], 1, 0, None),                     # one box per stage: the shape of the refusal tests
    # the compiled (4, 12) class on stages 1 to 3: nu + nx = 16, nb = 8 on every stage, an empty x_0
    "H": (5, [0, 12, 12, 12, 12, 12], [4] * 5, 4, 4, None),
    # the 16-wide tile edge with general constraints.  nb + ng slots per stage: 4 + 12 (a variable x_0 under general
    # constraints), 8 + 8 (nb 5, ng 7: both padded), 8 + 8 with nu = 0 and nx = 16, 8 + 8 with every box on an input,
    # and a last stage with nx = 16, nb = 0, ng = 16
    "E": (4, [4, 12, 16, 8, 16], [4, 4, 0, 8], [4, 2, 0, 8, 0], [0, 3, 8, 0, 0], [12, 7, 8, 8, 16]),
    # all boxes: stages 1 and 2 have nu = nx = 8 and nb = 16 (the 32 slots of lam / t full), stage 0 nx 4 and nb 12
    "B": (3, [4, 8, 8, 8], [8, 8, 8], [8, 8, 8, 0], [4, 8, 8, 8], None),
}
GENERAL = tuple(c for c, v in CASES.items() if v[5] is not None and any(v[5]))  # cases with a non-zero ng entry
ARGS = dict(mu0=2.0, mu_tol=1e-10, alpha_min=1e-8)
K_MAX = 50


def problems(case, seeds):
    return [IO.random_iface_problem(*CASES[case], seed=s) for s in seeds]


def make_solver(Ps, order, k_max=K_MAX):
    from hpmpc_amd.ocp_batch import OcpBatchSolver

    P = Ps[0]
    return OcpBatchSolver(P["N"], P["nx"], P["nu"], P["nb"], P["hidxb"], P["ng"], len(Ps), order=order, k_max=k_max)


def to_device(sv, flat):
    return {k: sv.torch.from_numpy(np.ascontiguousarray(v)).to(sv.dev) for k, v in flat.items()}


def pack_problems(sv, Ps, **kw):
    from hpmpc_amd.ocp_batch import flatten_problems

    sv.pack(to_device(sv, flatten_problems(Ps, sv.order)), **kw)


def expected_packed(sv, P):
    """One problem's BAbt, RSQrq, DCt, d arrays as to_qp builds them, each lib4 block whole (padding included) at the
    plan's offsets; the blocks tile the arrays, so comparing the arrays compares every element."""
    qp = IO.to_qp(P)
    N, s, o = P["N"], sv.sizes, sv.offsets
    out = dict(BAbt=np.full(max(s["BAbt"], 1), np.nan), RSQrq=np.full(max(s["RSQrq"], 1), np.nan),
               DCt=np.full(max(s["DCt"], 1), np.nan), d=np.zeros(32 * (N + 1)))
    used = dict(BAbt=0, RSQrq=0, DCt=0)
    for k in range(N + 1):
        blocks = [("RSQrq", qp.RSQrq[k])] + ([("BAbt", qp.BAbt[k])] if k < N else []) + \
                 ([("DCt", qp.DCt[k])] if P["ng"][k] else [])
        for name, blk in blocks:
            out[name][o[name][k]:o[name][k] + blk.size] = blk
            used[name] += blk.size
        n = 2 * qp.pnb(k) + 2 * qp.png(k)
        out["d"][32 * k:32 * k + n] = qp.d[k][:n]
    assert used == {k: s[k] for k in used}, (used, s)
    if s["DCt"] == 0:
        del out["DCt"]  # no DCt array
    return out


def packed_host(sv):
    sv.torch.cuda.synchronize()
    return {k: getattr(sv, k).cpu().numpy() for k in ("BAbt", "RSQrq", "DCt", "d") if sv.sizes[k]}


def compact(P, v):
    """Padded [lb pnb | ub pnb | lg png | ug png] per stage -> the wrappers' compact form."""
    out = []
    for k in range(P["N"] + 1):
        nb, ng = P["nb"][k], P["ng"][k]
        pnb, png = (nb + 3) // 4 * 4, (ng + 3) // 4 * 4
        out.append(np.r_[v[k][:nb], v[k][pnb:pnb + nb], v[k][2 * pnb:2 * pnb + ng],
                         v[k][2 * pnb + png:2 * pnb + png + ng]])
    return out


def oracle_ref(oracle, P, warm=None):
    """IO.ip_ocp over the oracle on the full space, plus the oracle's t (the IPM call ip_ocp makes, repeated) in the
    compact form."""
    N = P["N"]
    ref = IO.ip_ocp(oracle, P, N, k_max=K_MAX, mu0=ARGS["mu0"], mu_tol=ARGS["mu_tol"], warm=warm)
    kw = {}
    if warm is not None:
        kw = dict(warm_start=1, ux=[np.r_[warm["u"][k] if k < N else [], warm["x"][k]] for k in range(N + 1)])
    r = oracle.ipm(IO.to_qp(P), k_max=K_MAX, mu0=ARGS["mu0"], mu_tol=ARGS["mu_tol"], alpha_min=1e-8, **kw)
    assert (r["ret"], r["kk"]) == (ref["status"], ref["kk"])
    ref["t"] = compact(P, r["t"])
    return ref


def check(got, ref, keys=("u", "x", "pi", "lam", "t"), tag=""):
    """The gates of tests/test_gpu_iface.py: identical status and kk, the vectors at TOL_IPM relative to
    max(1, |ref|), inf_norm_res at 1e-9 absolute.  Returns the worst relative error of the vectors."""
    assert (got["status"], got["kk"]) == (ref["status"], ref["kk"]), tag
    worst = 0.0
    for key in keys:
        assert len(got[key]) == len(ref[key]), (tag, key)
        for k, (g, r) in enumerate(zip(got[key], ref[key])):
            g, r = np.asarray(g), np.asarray(r)
            assert g.shape == r.shape, (tag, key, k)
            if r.size:
                e = float(np.max(np.abs(g - r) / np.maximum(1.0, np.abs(r))))
                assert e <= TOL_IPM, (tag, key, k, e)
                worst = max(worst, e)
    np.testing.assert_allclose(got["inf_norm_res"], ref["inf_norm_res"], rtol=0, atol=1e-9)
    return worst


def solve_batch(Ps, order, warm=None):
    """pack -> ocp_ipm_batch -> finish on NaN-filled buffers; returns (solver, per-problem results).  warm: one
    dict(u=[..], x=[..]) per problem."""
    sv = make_solver(Ps, order)
    if warm is not None:
        warm = to_device(sv, dict(u=np.stack([np.concatenate(w["u"]) for w in warm]),
                                  x=np.stack([np.concatenate(w["x"]) for w in warm])))
    for x in (sv.BAbt, sv.RSQrq, sv.DCt, sv.d, sv.res, sv.u, sv.x, sv.pi_out, sv.lam_out, sv.t_out,
              sv.inf_norm_res):
        x.fill_(float("nan"))  # none of them needs initialisation
    pack_problems(sv, Ps, warm=warm)
    sv.solve(warm_start=0 if warm is None else 1, **ARGS)
    return sv, sv.results()

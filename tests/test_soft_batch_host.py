"""Host side of the batched soft-constraint IPM (hpmpc_amd/soft.py, include/hpmpc_mi355x.h): packing, layout and
the public symbols.  No GPU and no library load."""
import fnmatch
import os
import re

import numpy as np

from hpmpc_amd.soft import (mass_spring_soft, pack_soft_batch, soft_batch_layout, unpack_soft_batch,
                            unpack_soft_solution)

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NEW = ("hpmpc_mi355x_soft_plan_create", "hpmpc_mi355x_soft_plan_destroy", "hpmpc_mi355x_soft_sizes",
       "hpmpc_mi355x_soft_offsets", "hpmpc_mi355x_ipm_soft_batch")


def _mixed_batch():
    out = []
    for i, s in enumerate((0.2, 1.0, 3.5)):
        x0 = np.zeros(4)
        x0[0] = x0[1] = s
        out.append(mass_spring_soft(N=4, nx=4, nu=2, hard_last=2, Q_diag=1.0 + i, Zq=0.5 * i, zl=5.0 + i, x0=x0,
                                    time_variant=True, seed=3 + i, soft_bounds=(-1.0 - i, 1.0 + 0.5 * i)))
    return out


def test_pack_unpack_round_trip_is_exact():
    sqs = _mixed_batch()
    pk = pack_soft_batch(sqs)
    assert pk["BAbt"].shape == (3, pk["packB"]) and pk["RSQrq"].shape == (3, pk["packR"])
    assert not np.array_equal(pk["BAbt"][0], pk["BAbt"][1]) and not np.array_equal(pk["d"][0], pk["d"][2])
    back = unpack_soft_batch(sqs[0], pk)
    assert len(back) == len(sqs)
    for a, b in zip(sqs, back):
        assert a.N == b.N
        for f in ("nx", "nu", "nb", "ns", "ng"):
            assert np.array_equal(getattr(a, f), getattr(b, f))
        for f in ("idxb", "BAbt", "RSQrq", "d", "Z", "z"):
            for k, (x, y) in enumerate(zip(getattr(a, f), getattr(b, f))):
                assert np.array_equal(x, y), (f, k)


def test_pack_rejects_mismatched_sizes():
    import pytest

    with pytest.raises(ValueError):
        pack_soft_batch([mass_spring_soft(4, 4, 2), mass_spring_soft(4, 4, 2, hard_last=2)])


def test_layout_matches_the_reference_formulas():
    sq = mass_spring_soft(N=4, nx=4, nu=2, hard_last=2)
    assert int(sq.nb[4]) == 2 and int(sq.ns[4]) == 2  # hard and soft boxes on the last stage
    lay = soft_batch_layout(sq)
    r4 = lambda n: (int(n) + 3) // 4 * 4
    oD = oZ = oC = 0
    for k in range(sq.N + 1):
        pnb, pns = r4(sq.nb[k]), r4(sq.ns[k])
        assert (lay["oD"][k], lay["oZ"][k], lay["oC"][k]) == (oD, oZ, oC), k
        oD += 2 * pnb + 2 * pns  # d = [lb pnb | ub pnb | ls pns | us pns]
        oZ += 2 * pns            # Z / z = [lower pns | upper pns]
        oC += 2 * pnb + 4 * pns  # lam / t = [lo pnb | up pnb | 4 x pns]
    sz = lay["sizes"]
    assert (sz["d"], sz["Z"], sz["C"], sz["ux"], sz["N"]) == (oD, oZ, oC, 16 * (sq.N + 1), sq.N)
    # stages: nb = 2,2,2,2,2 (pnb 4), ns = 0,4,4,4,2 (pns 0,4,4,4,4)
    assert list(lay["oD"]) == [0, 8, 24, 40, 56] and list(lay["oC"]) == [0, 8, 32, 56, 80]
    assert sz["ws"] % 32 == 0 and sz["ws"] >= 352 * 5 + 7 * 16 * 5 + 4 * sz["C"]


def test_unpack_solution_shapes():
    sq = mass_spring_soft(N=4, nx=4, nu=2, hard_last=2)
    lay = soft_batch_layout(sq)
    P, k_max = 2, 6
    rng = np.random.default_rng(0)
    ux, pi = rng.standard_normal((P, 5, 16)), rng.standard_normal((P, 5, 16))
    lam, t = rng.standard_normal((P, lay["sizes"]["C"])), rng.standard_normal((P, lay["sizes"]["C"]))
    stat = rng.standard_normal((P, 5 * k_max))
    res = unpack_soft_solution(sq, ux, pi, lam, t, np.array([3, 6]), np.array([0, 1]), stat)
    assert [r["kk"] for r in res] == [3, 6] and [r["ret"] for r in res] == [0, 1]
    assert res[0]["stat"].shape == (15,) and np.array_equal(res[1]["stat"], stat[1])
    for p, r in enumerate(res):
        assert len(r["ux"]) == 5 and len(r["pi"]) == 4 and len(r["lam"]) == 5 and len(r["t"]) == 5
        for k in range(5):
            assert np.array_equal(r["ux"][k], ux[p, k, :sq.nux(k)])
            o = lay["oC"][k]
            assert np.array_equal(r["lam"][k], lam[p, o:o + sq.ncv(k)])
            assert np.array_equal(r["t"][k], t[p, o:o + sq.ncv(k)])
        assert np.array_equal(r["pi"][2], pi[p, 2, :4])


def test_header_declares_and_export_map_lists_the_new_functions():
    header = open(os.path.join(ROOT, "include", "hpmpc_mi355x.h")).read()
    header = re.sub(r"/\*.*?\*/", "", header, flags=re.S)
    assert "typedef struct hpmpc_mi355x_soft_plan hpmpc_mi355x_soft_plan;" in header
    for name in NEW:
        assert re.search(r"\b%s\s*\(" % name, header), name
    m = re.search(r"\bint\s+hpmpc_mi355x_ipm_soft_batch\s*\(([^;]*)\)\s*;", header)
    args = [a.strip() for a in m.group(1).replace("\n", " ").split(",")]
    assert len(args) == 25 and args[0].startswith("const hpmpc_mi355x_soft_plan") and args[-1] == "void *stream"
    emap = open(os.path.join(ROOT, "hpmpc_amd", "csrc", "exports.map")).read()
    emap = re.sub(r"/\*.*?\*/", "", emap, flags=re.S)
    glob = re.search(r"global:(.*?)local:", emap, flags=re.S).group(1)
    patterns = [p.strip() for p in glob.split(";") if p.strip()]
    for name in NEW:
        assert any(fnmatch.fnmatchcase(name, p) for p in patterns), name

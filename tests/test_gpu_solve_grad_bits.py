"""
The fused solve + gradient kernel bit for bit against a record of the commit before its prologue, the fold's addressing, the tile
wavefronts' addressing and the solver's prologue were rewritten: V, grad V, status and the v workspace of plan.eval (delta = 0 and
delta != 0) and of plan.solve_grad fed from a Phi record, for allocations that take the solver's rare passes, on the smallest
plans that reach each path (tests/solve_grad_bits_cases.py lists them); x, m, V and status of three steps of the single-output
update tail (bluest_plan_eval_ma).  The record, tests/golden/solve_grad_bits_parent.npz, was written by
tools/gen_golden_solve_grad_bits.py from that commit on the MI355X; the inputs are seeded, the file holds results only.

np.array_equal throughout, doubles compared as their bit patterns (a NaN of a singular solve must stay that NaN): the rewrite
changes where addresses are computed and how the diagonal gets its delta, never which values are added in which order.
"""
import ctypes
import os

import numpy as np
import pytest

import solve_grad_bits_cases as sgc
from conftest import golden

FIXTURE = "solve_grad_bits_parent.npz"
OK, NO_MODEL0 = 0, 2      # BLUEST_EVAL_OK, BLUEST_EVAL_NO_MODEL0 (include/bluest_hip.h)


@pytest.fixture(scope="module")
def record():
    return golden(FIXTURE)


def test_record_is_complete(record):
    """CPU: every case has every array of every call, the file stays within the size a committed fixture may have, and the record
    shows the statuses the allocations are made for"""
    for name in sgc.NAMES:
        for key in sgc.keys(name):
            assert key in record and record[key].size > 0, key
            assert record[key].dtype in (np.int64, np.int32), key
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", FIXTURE)) < 400 * 1024
    for name in sgc.NAMES[:-1]:
        assert (record[name + "/ok/st"] == OK).all() and (record[name + "/no3/st"] == OK).all(), name
        assert (record[name + "/ok_d/st"] == OK).all() and (record[name + "/ok_rec/st"] == OK).all(), name
        assert (record[name + "/no0/st"] == NO_MODEL0).all(), name
        for a, b in (("ok", "ok_rec"),):          # the record-fed launch solves the same Phi
            assert np.array_equal(record["%s/%s/var" % (name, a)], record["%s/%s/var" % (name, b)]), name
        assert not np.array_equal(record[name + "/ok/var"], record[name + "/ok_d/var"]), name       # delta took effect
    assert all((record["ma_n6_o1/step%d/st" % s] == OK).all() for s in range(sgc.MA_STEPS))


def test_cases_reach_their_paths():
    """CPU: what the case table claims, from the layout rules restated in solve_grad_bits_cases (layout_tiles, the NT and KU
    dispatchers, layout_fold_reg through step_bits_cases) and from the allocations themselves"""
    import step_bits_cases as sbc
    lay, prob = {}, {}
    for name in sgc.NAMES:
        prob[name] = sgc.problem(name)
        lay[name] = sgc.layout(prob[name])
        assert lay[name]["tiles_per_wg"] < lay[name]["fused_tpb"], name            # wavefronts that only fold, in every case
    assert lay["reg_n6_o2"]["bpo"] == 3 and lay["reg_n8_o3"]["bpo"] == 5          # equal workgroups per output, two sizes
    assert lay["ragged_o2"]["wgs"] == [3, 2] and lay["ragged_o2"]["bpo"] == 0     # output and `first` from the descriptor
    for name in ("reg_n6_o2", "reg_n8_o3", "pads_n10_o1", "extra_n18_o2", "generic_n14", "ma_n6_o1"):
        p = prob[name]
        assert sbc.regular_fold(p["n"], p["groups"], p["n_out"]), name
    p = prob["rowrag_o2"]
    assert not sbc.regular_fold(p["n"], p["groups"], p["n_out"]) and p["env"] == {"BLUEST_NO_REGULAR_FOLD": "1"}
    assert lay["reg_n8_o3"]["nt"] == prob["reg_n8_o3"]["n"]                       # no pads
    for name, nt in (("reg_n6_o2", 8), ("pads_n10_o1", 12), ("rowrag_o2", 12), ("extra_n18_o2", 20)):
        assert lay[name]["nt"] == nt > prob[name]["n"], name                      # pads
    assert lay["extra_n18_o2"]["extra_rows"] == 4 and all(lay[k]["extra_rows"] == 0 for k in sgc.NAMES if k != "extra_n18_o2")
    assert lay["generic_n14"]["kmax"] == 13 and lay["generic_n14"]["ku"] == 12 and lay["generic_n14"]["fused_tpb"] == 7
    assert lay["rowrag_o2"]["kmax"] == 11 and lay["rowrag_o2"]["ku"] == 12       # unrolled tile paths of the widest instantiation
    assert all(lay[k]["kmax"] <= 5 and lay[k]["ku"] == 5 and lay[k]["fused_tpb"] == 15 for k in sgc.NAMES if k not in ("generic_n14", "rowrag_o2"))
    assert lay["ma_n6_o1"]["wgs"] == [3] and prob["ma_n6_o1"]["outs"][0]["mapping"] is None
    for name in sgc.NAMES[:-1]:
        p = prob[name]
        for kind, want in (("ok", None), ("no3", 3), ("no0", 0), ("tiny2", None)):
            for m1, m2 in sgc.masks(p, kind):
                if kind == "tiny2":      # model 2 is in v's system and not in V's: the second pass
                    assert not m1[2] and m2[2] and m1.sum() == p["n"] - 1 and m2.all(), (name, kind)
                else:
                    assert (m1 == m2).all() and [i for i in range(p["n"]) if not m1[i]] == ([] if want is None else [want]), (name, kind)
    assert {c[2] for c in sgc.CALLS} == {0.0, sgc.DELTA} and any(c[3] for c in sgc.CALLS)


def _v_peeker(torch, plan):
    from bluest_amd._lib import check
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    v = ctypes.c_void_p()
    check(plan.lib.bluest_plan_v_workspace(plan._h, ctypes.byref(v), None))

    def peek():
        torch.cuda.synchronize()
        out = np.empty(plan.n_out * plan.N, dtype=np.float64)
        assert hip.hipMemcpy(out.ctypes.data, v.value, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
        return out
    return peek


@pytest.mark.gpu
@pytest.mark.parametrize("name", sgc.NAMES)
def test_solve_grad_bits(record, monkeypatch, name):
    import torch
    from bluest_amd.plan import Plan
    assert torch.cuda.is_available(), "these tests need the MI355X"
    p = sgc.problem(name)
    for k in sgc.ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, val in p["env"].items():
        monkeypatch.setenv(k, val)
    plan = Plan(p["n"], p["L"], p["outs"])
    cfg, lay = plan.launch_config(1), sgc.layout(p)
    for key in ("nt", "fused_tpb", "tiles_per_wg"):
        assert cfg[key] == lay[key], (name, key, cfg, lay)
    assert cfg["solve_grad_ku"] == lay["ku"] and cfg["matfree"] == 0 and cfg["tiles_per_wg"] < cfg["fused_tpb"], (name, cfg)
    got = sgc.record(plan, name, p, _v_peeker(torch, plan))
    assert sorted(got) == sorted(sgc.keys(name))
    for key, a in got.items():
        want = record[key]
        assert a.dtype == want.dtype and a.shape == want.shape, key
        print("%-28s %6d entries, %d differ" % (key, a.size, int((a != want).sum())))
        assert np.array_equal(a, want), key

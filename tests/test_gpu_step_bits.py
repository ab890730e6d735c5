"""
The evaluation step bit for bit against a record of the commit before its cross-lane reductions and prologues were rewritten:
plan.phi, plan.eval (V, grad V, status) of one allocation and plan.eval of two, for the smallest plans that reach each path of
the Phi kernels and of the fold (tests/step_bits_cases.py lists them).  The record, tests/golden/step_bits_parent.npz, was written
by tools/gen_golden_step_bits.py from that commit on the MI355X; the inputs are seeded, the file holds results only.

np.array_equal throughout (NaN-free results: every status of the record is OK): the rewrite changes how lanes exchange values,
never which values are added in which order.
"""
import os

import numpy as np
import pytest

import step_bits_cases as sbc
from conftest import golden

ENV_KEYS = ("BLUEST_MATFREE", "BLUEST_COLS32", "BLUEST_TILE_NT", "BLUEST_NO_REGULAR_FOLD")


@pytest.fixture(scope="module")
def record():
    return golden("step_bits_parent.npz")


def test_record_is_complete(record):
    """CPU: every case has its eight arrays, within the size a committed fixture may have; no NaN hides a difference"""
    for name in sbc.NAMES:
        for what in ("phi1", "var1", "grad1", "st1", "phi2", "var2", "grad2", "st2"):
            a = record["%s/%s" % (name, what)]
            assert a.size > 0 and not np.isnan(a.astype(np.float64)).any(), (name, what)
        assert not record[name + "/st1"].any() and not record[name + "/st2"].any(), name
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "step_bits_parent.npz")) < 400 * 1024


def test_cases_reach_their_paths():
    """CPU: what the case table claims about the fold and the chunk length, from the layout rules restated in step_bits_cases"""
    regular, iters = {}, {}
    for name in sbc.NAMES:
        n, _, outs, _, _, expect, reg = sbc.problem(name)
        regular[name], iters[name] = reg, sbc.row_chunks(n, outs[0]["groups"])[1]
        assert iters[name] == expect["iters"], name
    assert not regular["rowrag_o2"] and not regular["rowrag_o1"] and not regular["long_o1"]
    assert all(regular[k] for k in ("shared_o3", "plain_o1", "shared_o8", "cols32_o1"))
    assert iters["long_o1"] > 1


@pytest.mark.gpu
@pytest.mark.parametrize("name", sbc.NAMES)
def test_step_bits(record, monkeypatch, name):
    import torch
    from bluest_amd.plan import Plan
    assert torch.cuda.is_available(), "these tests need the MI355X"
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    n, Lg, outs, m1, M2, expect, regular = sbc.problem(name)
    if not regular:
        monkeypatch.setenv("BLUEST_NO_REGULAR_FOLD", "1")      # (the layout decides the same; this makes the descriptor fold certain)
    plan = Plan(n, Lg, outs, max_candidates=2)
    cfg = plan.launch_config(1)
    for key, want in expect.items():
        assert cfg[key] == want, (name, key, cfg)
    if name == "long_o1":
        assert cfg["iters"] > 1
    if name == "cols32_o1":
        assert Lg > 65536 and outs[0]["mapping"] is not None and cfg["cols16"] == 0
    got = sbc.record(plan, name, m1, M2)
    for key, a in got.items():
        want = record[key]
        assert a.dtype == want.dtype and a.shape == want.shape, key
        diff = int((a != want).sum())
        print("%-18s %8d entries, %d differ" % (key, a.size, diff))
        assert np.array_equal(a, want), key

"""
k_phi_chunks_shared<OB> at every OB, forced with BLUEST_PHI_OB (read per plan at finalize): the evaluation step keeps its bits
whichever OB streams the chunks.  The transposed reduction of the OB sums (wave_sum_multi) pairs the lanes of every output as
the single-sum tail did, so nothing may differ, not in the last bit.

  * shared_o3, shared_o8, rowrag_o2 of tests/step_bits_cases.py at OB = 4 and 8 against tests/golden/step_bits_parent.npz
    (plan.phi and plan.eval of one allocation and of two): tail blocks with 1 (3 outputs, OB 4), 5 (3 outputs, OB 8), 2 and 6
    (2 outputs) clamped outputs, the slot table (regular fold) and the descriptor fold.  After the OB = 8 run on shared_o3 a plan
    at OB = 2 still gives the record's Phi: a clamped output that stored anything would have written into a neighbour's slots
    of blocks the cache hands on.
  * int32 columns: n = 8 / k <= 3, 5 outputs, L_global = 70 000 with a mapping; Phi record and eval of one allocation and of a batch
    of three, equal between OB = 2, 4 and 8.
  * iters = 2 in the shared kernel: every subset of 16 models, 2 outputs (the smallest all-subsets plan with more than 64 x 256
    entries in a row); Phi record and eval of one allocation, equal between OB = 2, 4 and 8, the gradient on every 61st entry.

np.array_equal throughout; every status is OK, so no NaN hides a difference.
"""
import numpy as np
import pytest

import step_bits_cases as sbc
from conftest import golden

ENV_KEYS = ("BLUEST_MATFREE", "BLUEST_COLS32", "BLUEST_TILE_NT", "BLUEST_NO_REGULAR_FOLD", "BLUEST_PHI_OB")


@pytest.fixture(scope="module")
def record():
    return golden("step_bits_parent.npz")


def _clean_env(monkeypatch, ob):
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    monkeypatch.setenv("BLUEST_PHI_OB", str(ob))


def _plan(monkeypatch, ob, n, Lg, outs, max_candidates, regular=True):
    from bluest_amd.plan import Plan
    _clean_env(monkeypatch, ob)
    if not regular:
        monkeypatch.setenv("BLUEST_NO_REGULAR_FOLD", "1")      # (the layout decides the same; this makes the descriptor fold certain)
    plan = Plan(n, Lg, outs, max_candidates=max_candidates)
    cfg = plan.launch_config(1)
    assert cfg["phi_ob"] == ob, cfg
    assert plan.launch_config(max_candidates)["phi_ob"] == ob
    return plan, cfg


def test_cases_clamp_what_they_claim():
    """CPU: outputs beyond n_out in the last block of each forced run"""
    clamped = {(name, ob): -sbc.problem(name)[2].__len__() % ob for name in ("shared_o3", "shared_o8", "rowrag_o2") for ob in (4, 8)}
    assert clamped[("shared_o3", 4)] == 1 and clamped[("shared_o3", 8)] == 5
    assert clamped[("rowrag_o2", 4)] == 2 and clamped[("rowrag_o2", 8)] == 6
    assert clamped[("shared_o8", 4)] == 0 and clamped[("shared_o8", 8)] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("name", ["shared_o3", "shared_o8", "rowrag_o2"])
def test_forced_ob_against_the_record(record, monkeypatch, name):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    n, Lg, outs, m1, M2, expect, regular = sbc.problem(name)
    for ob in (4, 8):
        plan, cfg = _plan(monkeypatch, ob, n, Lg, outs, 2, regular)
        assert cfg["cols16"] == expect["cols16"] and cfg["iters"] == expect["iters"] and cfg["path"] == expect["path"]
        got = sbc.record(plan, name, m1, M2)
        for key, a in got.items():
            want = record[key]
            assert a.dtype == want.dtype and a.shape == want.shape, (key, ob)
            print("OB = %d  %-18s %8d entries, %d differ" % (ob, key, a.size, int((a != want).sum())))
            assert np.array_equal(a, want), (key, ob)
        del plan
    if name == "shared_o3":
        plan, _ = _plan(monkeypatch, 2, n, Lg, outs, 2, regular)
        phi = plan.phi(m1).cpu().numpy()
        assert np.array_equal(phi, record[name + "/phi1"])


def _between_obs(monkeypatch, n, Lg, outs, ms, max_candidates, grad_stride=1):
    """phi and eval of every allocation (batch) of ms at OB = 2, 4, 8: all equal to OB = 2's; returns the launch configurations"""
    first, cfgs = None, {}
    for ob in (2, 4, 8):
        plan, cfgs[ob] = _plan(monkeypatch, ob, n, Lg, outs, max_candidates)
        got = {}
        for i, m in enumerate(ms):
            got["phi%d" % i] = plan.phi(m).cpu().numpy()
            v, g, st = plan.eval(m)
            got["var%d" % i], got["grad%d" % i], got["st%d" % i] = v.cpu().numpy(), g.cpu().numpy()[..., ::grad_stride].copy(), st.cpu().numpy()
            assert not got["st%d" % i].any(), (ob, i)
        del plan
        if first is None:
            first = got
            for key, a in got.items():
                assert a.size > 0 and not np.isnan(a.astype(np.float64)).any(), key
            continue
        for key, a in got.items():
            print("OB = %d against 2  %-8s %8d entries, %d differ" % (ob, key, a.size, int((a != first[key]).sum())))
            assert a.shape == first[key].shape and np.array_equal(a, first[key]), (key, ob)
    return cfgs


def _outputs(n, groups, n_out, mapping):
    from bluest_amd import synth
    return [{"K": len(groups), "sizes": [len(g) for g in groups], "groups": [g.copy() for g in groups],
             "C": synth.wishart_covariance(n, o)[0], "mapping": mapping} for o in range(n_out)]


@pytest.mark.gpu
def test_int32_columns_between_obs(monkeypatch):
    import torch
    from bluest_amd import synth
    assert torch.cuda.is_available(), "these tests need the MI355X"
    n, Lg = 8, 70000
    groups = synth.all_groups(n, 3)
    L = int(sum(len(g) for g in groups))
    rng = np.random.RandomState(4107)
    mapping = np.sort(rng.choice(Lg, L, replace=False)).astype(np.int64)
    mapping[-1] = Lg - 1                                       # a column index above 65 535 is really stored
    outs = _outputs(n, groups, 5, mapping)
    m1 = 10.0 * rng.rand(Lg)
    M3 = np.stack([0.5 + rng.rand(Lg), (0.5 + rng.rand(Lg)) * (rng.rand(Lg) < 0.6), 3.0 * rng.rand(Lg) + 0.01])
    M3[1, mapping[:n]] = 0.75                                  # the singletons stay sampled
    cfgs = _between_obs(monkeypatch, n, Lg, outs, [m1, M3], 3)
    assert all(c["cols16"] == 0 and c["iters"] == 1 for c in cfgs.values())


@pytest.mark.gpu
def test_two_blocks_per_chunk_between_obs(monkeypatch):
    import torch
    from bluest_amd import synth
    assert torch.cuda.is_available(), "these tests need the MI355X"
    n = 16
    groups = synth.all_groups(n, n)
    L = int(sum(len(g) for g in groups))
    outs = _outputs(n, groups, 2, None)
    m1 = 10.0 * np.random.RandomState(4108).rand(L)
    cfgs = _between_obs(monkeypatch, n, L, outs, [m1], 1, grad_stride=61)
    assert all(c["iters"] == 2 and c["cols16"] == 1 for c in cfgs.values())

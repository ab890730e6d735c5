"""
The entry code of the Phi kernels (csrc/plan.hip: k_phi_chunks, k_phi_chunks_shared<2|4|8>): the opening sweep issues the column
load and the first output's value loads in front of everything only the stores need, the later outputs' bases and the store's
bookkeeping are formed once behind them, and the loops over the 256-blocks and the candidates follow that sweep.  The kernels
behind them in the step (k_solve_grad, k_solve_from_chunks + k_grad_tiles) read what they store, on every path of the fold.
What moved must not change a bit, so every check here is np.array_equal on bit patterns.

Plans, the smallest that reach each path whose entry code moved:
  * n = 6 with every group up to size 3 (NT = 8, so Phi has pads that the fold must find cleared) and 1, 3, 5, 8 outputs: the
    plain kernel; the tail block with a clamped base at OB = 2 (3 outputs) and at OB = 4 (5 outputs, forced); full blocks at OB = 4 and OB = 8 (8 outputs, forced); the 3-output plan again with the
    descriptor fold; the ragged 3-output plan, whose k_solve_grad takes its output from a tile descriptor (the plans of
    tests/test_gpu_step_args.py);
  * long_o1 of tests/step_bits_cases.py: n = 16, every subset, 32 768 entries per diagonal row, so iters = 2 (the loop behind the
    opening sweep) and the descriptor fold's second sweep; shared_o3 and rowrag_o2 of the same table.

Checks per plan
  * a batch of three allocations (n_cand = 3: the work behind the opening sweep's loads is done once, the candidates' loop reuses
    it; k_solve_from_chunks folds with fold_rows, k_grad_tiles forms the gradient) against the three evaluated one at a time
    (k_solve_grad: the regular or the descriptor fold);
  * the record-fed launch of k_solve_grad against the partial-fed one on the same m;
  * gate open: the same bits as without a gate; gate closed: var, grad and status keep what was in them;
  * plans that differ in OB alone against each other;
  * the step_bits cases against the parent's record, tests/golden/step_bits_parent.npz, for one allocation and for two.
"""
import numpy as np
import pytest

import step_bits_cases as sbc
import test_gpu_step_args as tsa
from conftest import golden

ENV_KEYS = tsa.ENV_KEYS
# plan of tests/test_gpu_step_args.py -> what it is here for
ARGS_PLANS = {
    "n6_o1": "plain kernel, slot table, pads",
    "n6_o3": "OB 2, tail block with a clamped base",
    "n6_o5_ob4": "OB 4, tail block with three clamped bases",
    "n6_o8_ob4": "OB 4, full blocks",
    "n6_o8_ob8": "OB 8, one full block",
    "n6_o8": "OB 2, full blocks (the OB-alone comparison)",
    "n6_o5_ob8": "OB 8, three clamped bases (the OB-alone comparison)",
    "n6_o3_desc": "descriptor fold with pads, no slot table",
    "n6_o3_ragged": "output from the tile descriptor (bpo = 0)",
}
SAME_BUT_OB = [("n6_o8", "n6_o8_ob4"), ("n6_o8", "n6_o8_ob8"), ("n6_o5_ob4", "n6_o5_ob8")]
BITS_CASES = ("shared_o3", "rowrag_o2", "long_o1")
SENTINEL = -7.25


def _bits(a):
    a = a.cpu().numpy() if hasattr(a, "cpu") else np.asarray(a)
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what):
    a, b = _bits(a), _bits(b)
    assert a.shape == b.shape and a.dtype == b.dtype, what
    diff = int((a != b).sum())
    print("%-40s %8d entries, %d differ" % (what, a.size, diff))
    assert diff == 0, what


def allocations(L, n, seed):
    """(3, L): dense, sparse with the singletons sampled, dense small"""
    rng = np.random.RandomState(seed)
    M = 0.5 + rng.rand(3, L)
    M[1] *= rng.rand(L) < 0.7
    M[1, :n] = 0.75
    M[2] *= 0.1
    return M


def test_plans_are_the_ones_meant():
    """CPU: the plans named above exist with the outputs, OB and fold the list claims, and the n = 6 plans have pads"""
    import solve_grad_bits_cases as sgc
    for name in ARGS_PLANS:
        p = tsa.problem(name)
        lay = sgc.layout(dict(n=p["n"], n_out=p["n_out"], local=p["local"], groups=p["groups"]))
        assert lay["nt"] > p["n"] == 6, name
        assert (lay["bpo"] == 0) == (name == "n6_o3_ragged"), name
    assert sorted(tsa.problem(n)["n_out"] for n in ("n6_o1", "n6_o3", "n6_o5_ob4", "n6_o8_ob8")) == [1, 3, 5, 8]
    assert [tsa.problem(n)["want_ob"] for n in ("n6_o1", "n6_o3", "n6_o5_ob4", "n6_o8_ob4", "n6_o8_ob8")] == [0, 2, 4, 4, 8]
    assert tsa.problem("n6_o3_desc")["env"] == {"BLUEST_NO_REGULAR_FOLD": "1"}
    for a, b in SAME_BUT_OB:
        pa, pb = tsa.problem(a), tsa.problem(b)
        assert pa["n_out"] == pb["n_out"] and pa["L"] == pb["L"] and pa["want_ob"] != pb["want_ob"]
    n, _, outs, _, _, expect, regular = sbc.problem("long_o1")
    assert expect["iters"] == 2 == sbc.row_chunks(n, outs[0]["groups"])[1] and not regular


def _plan(p, monkeypatch, max_candidates=3):
    import torch
    from bluest_amd.plan import Plan
    assert torch.cuda.is_available(), "these tests need the MI355X"
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in p["env"].items():
        monkeypatch.setenv(k, v)
    return Plan(p["n"], p["L"], p["outs"], max_candidates=max_candidates)


_singles = {}      # plan name -> [(var, grad, status) host arrays of its three allocations, one at a time]


def _evaluate_singles(name, plan, M):
    if name not in _singles:
        _singles[name] = [tuple(t.cpu().numpy() for t in plan.eval(M[c])) for c in range(len(M))]
    return _singles[name]


@pytest.mark.gpu
@pytest.mark.parametrize("name", list(ARGS_PLANS))
def test_entry_paths_agree(monkeypatch, name):
    import torch
    from bluest_amd._lib import check
    p = tsa.problem(name)
    plan = _plan(p, monkeypatch)
    assert plan.launch_config(1)["phi_ob"] == p["want_ob"] == plan.launch_config(3)["phi_ob"]
    assert plan.launch_config(1)["path"] == 1 and plan.launch_config(3)["path"] == 0
    M = allocations(p["L"], p["n"], 9300 + p["n_out"])
    singles = _evaluate_singles(name, plan, M)
    assert all(not s[2].any() for s in singles)
    # n_cand = 3 against one at a time
    vb, gb, sb = plan.eval(M)
    for c in range(3):
        _same(vb[c:c + 1], singles[c][0], "%s batch V %d" % (name, c))
        _same(gb[c:c + 1], singles[c][1], "%s batch grad %d" % (name, c))
        _same(sb[c:c + 1], singles[c][2], "%s batch status %d" % (name, c))
    # record-fed against partial-fed
    for c in range(3):
        v, g, st = plan.solve_grad(plan.phi(M[c]))
        _same(v, singles[c][0], "%s record V %d" % (name, c))
        _same(g, singles[c][1], "%s record grad %d" % (name, c))
        _same(st, singles[c][2], "%s record status %d" % (name, c))
    # the gate, open and closed
    enable = torch.ones(1, dtype=torch.int32, device=plan.device)
    out = (torch.full((1, plan.n_out), SENTINEL, dtype=torch.float64, device=plan.device),
           torch.full((1, plan.grad_len), SENTINEL, dtype=torch.float64, device=plan.device),
           torch.full((1, plan.n_out), -3, dtype=torch.int32, device=plan.device))
    with torch.cuda.device(plan.device):
        check(plan.lib.bluest_plan_set_gate(plan._h, enable.data_ptr(), 0))
    try:
        plan.eval(M[1], out=out)
        _same(out[0], singles[1][0], "%s gate open V" % name)
        _same(out[1], singles[1][1], "%s gate open grad" % name)
        _same(out[2], singles[1][2], "%s gate open status" % name)
        enable.zero_()
        for t, x in zip(out, (SENTINEL, SENTINEL, -3)):
            t.fill_(x)
        plan.eval(M[0], out=out)
        torch.cuda.synchronize(plan.device)
        assert (out[0] == SENTINEL).all() and (out[1] == SENTINEL).all() and (out[2] == -3).all(), "%s gate closed" % name
        enable.fill_(1)
        plan.eval(M[0], out=out)
        _same(out[0], singles[0][0], "%s gate reopened V" % name)
        _same(out[1], singles[0][1], "%s gate reopened grad" % name)
    finally:
        with torch.cuda.device(plan.device):
            check(plan.lib.bluest_plan_set_gate(plan._h, None, 0))


@pytest.mark.gpu
@pytest.mark.parametrize("a,b", SAME_BUT_OB)
def test_ob_alone_changes_nothing(monkeypatch, a, b):
    pa, pb = tsa.problem(a), tsa.problem(b)
    M = allocations(pa["L"], pa["n"], 9300 + pa["n_out"])
    res = []
    for name, p in ((a, pa), (b, pb)):
        plan = _plan(p, monkeypatch)
        assert plan.launch_config(1)["phi_ob"] == p["want_ob"]
        res.append((_evaluate_singles(name, plan, M), plan.phi(M).cpu().numpy()))
    _same(res[0][1], res[1][1], "%s / %s Phi records" % (a, b))
    for c in range(3):
        for i, what in enumerate(("V", "grad", "status")):
            _same(res[0][0][c][i], res[1][0][c][i], "%s / %s %s %d" % (a, b, what, c))


@pytest.fixture(scope="module")
def parent_record():
    return golden("step_bits_parent.npz")


@pytest.mark.gpu
@pytest.mark.parametrize("name", BITS_CASES)
def test_against_the_parent_record(parent_record, monkeypatch, name):
    """one allocation (k_solve_grad) and two (the candidates' loop, k_solve_from_chunks) against the parent's bits, and the
    record-fed launch against the partial-fed one"""
    import torch
    from bluest_amd.plan import Plan
    assert torch.cuda.is_available(), "these tests need the MI355X"
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    n, Lg, outs, m1, M2, expect, regular = sbc.problem(name)
    if not regular:
        monkeypatch.setenv("BLUEST_NO_REGULAR_FOLD", "1")
    plan = Plan(n, Lg, outs, max_candidates=2)
    assert plan.launch_config(1)["iters"] == expect["iters"]
    got = sbc.record(plan, name, m1, M2)
    for key, arr in got.items():
        _same(arr, parent_record[key], key)
    s = sbc.GRAD_STRIDE.get(name, 1)
    v, g, st = plan.solve_grad(plan.phi(m1))
    _same(v, parent_record[name + "/var1"], name + " record-fed V")
    _same(g.cpu().numpy()[:, ::s].copy(), parent_record[name + "/grad1"], name + " record-fed grad")
    _same(st, parent_record[name + "/st1"], name + " record-fed status")

"""
The evaluation step's kernels after their argument lists were reordered for kernarg preload (csrc/plan.hip: k_phi_chunks,
k_phi_chunks_shared<2|4|8>, k_solve_grad): every launch site with the new order, on the smallest plans that reach it, and the
max|m| that the Phi pass hands to the fold, flag by flag.

Plans (PLANS): n = 6 with every group up to size 3 (NT = 8: pads) and 1, 2, 3, 5, 8 outputs -- the plain kernel, OB = 2 with and
without a tail block, OB = 4 and 8 forced through BLUEST_PHI_OB --, all of them again with BLUEST_NO_REGULAR_FOLD=1 (descriptor
fold, no slot table) and with BLUEST_COLS32=1; one ragged 3-output plan (outputs 1 and 2 without the triples: 3, 2 and 2
workgroups, so k_solve_grad takes its output from the tile descriptor; not shared, so the slot numbers run over all outputs);
one n = 20 / k <= 3 plan (N = NT, no pads).

For each plan
  * one evaluation, each row of a batch of three handed over with m_stride > L (the padding poisoned with NaN and found
    untouched), the split path phi -> solve -> grad and the record-fed bluest_plan_solve_grad agree bit for bit in V, grad V and
    status;
  * allocation vectors with ONE non-zero entry -- 2e-6, 5e-7, 0.06 or 0.04 in the first and the last group of every size (a
    singleton, groups with model 0, groups of the largest size) -- give the three flag groups of the Phi record (per model
    "touched above 1e-6", "touched at all", and "max|m| >= 0.05") that a numpy restatement expects, from a batch and one at a
    time, and the status that follows from them (OK / INF / NO_MODEL0), from eval() too.  The flags come from the maxima in the
    slots of the diagonal destinations alone: a Phi pass that kept them for the wrong slots would drop a group's only maximum.

Equality throughout (np.array_equal on the bit patterns): nothing arithmetic differs between the paths.
"""
import numpy as np
import pytest

import solve_grad_bits_cases as sgc

ENV_KEYS = ("BLUEST_MATFREE", "BLUEST_COLS32", "BLUEST_TILE_NT", "BLUEST_NO_REGULAR_FOLD", "BLUEST_PHI_OB")
OK, INF, NO_MODEL0 = 0, 1, 2
VALUES = (2.0e-6, 5.0e-7, 0.06, 0.04)
PAD = 5            # doubles between the rows of the strided batch

#        name         n   kmax  n_out  forced OB (0: the plan's own)  phi_ob expected
BASE = [
    ("n6_o1",        6,  3,    1,     0,                             0),      # the plain kernel
    ("n6_o2",        6,  3,    2,     0,                             2),      # OB 2 without a tail block
    ("n6_o3",        6,  3,    3,     0,                             2),      # OB 2 with a tail block
    ("n6_o8",        6,  3,    8,     0,                             2),
    ("n6_o3_ob4",    6,  3,    3,     4,                             4),      # one block, one clamped output
    ("n6_o5_ob4",    6,  3,    5,     4,                             4),
    ("n6_o8_ob4",    6,  3,    8,     4,                             4),
    ("n6_o5_ob8",    6,  3,    5,     8,                             8),
    ("n6_o8_ob8",    6,  3,    8,     8,                             8),
]
VARIANTS = [("", {}), ("_desc", {"BLUEST_NO_REGULAR_FOLD": "1"}), ("_c32", {"BLUEST_COLS32": "1"})]
#        name, n, kmax, n_out, forced OB, phi_ob expected, env, ragged: every base plan under every variant, then the two others
PLANS = [(row[0] + tag,) + row[1:] + (env, False) for tag, env in VARIANTS for row in BASE]
PLANS += [
    ("n6_o3_ragged", 6,  3,    3,     0,                             0,               {},  True),
    ("n20_o2",       20, 3,    2,     0,                             2,               {},  False),
]
NAMES = [c[0] for c in PLANS]


def problem(name):
    """dict: n, L, n_out, groups (global, by size), local (per output: its groups by size), first (global index of each size's
    first group), outs (for Plan()), env, ob"""
    from bluest_amd import synth
    _, n, kmax, n_out, ob, want_ob, env, ragged = PLANS[NAMES.index(name)]
    G = synth.all_groups(n, kmax)
    sizes = np.array([len(g) for g in G])
    L = int(sizes.sum())
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    outs, local = [], []
    for o in range(n_out):
        gl = [g if (not ragged or o == 0 or k <= 2) else g[:0] for k, g in enumerate(G, start=1)]
        mapping = np.concatenate([f + np.arange(len(g)) for f, g in zip(first, gl)]).astype(np.int64) if ragged else None
        outs.append({"K": len(G), "sizes": [len(g) for g in gl], "groups": [g.copy() for g in gl],
                     "C": synth.wishart_covariance(n, o)[0], "mapping": mapping})
        local.append(gl)
    env = dict(env)
    if ob:
        env["BLUEST_PHI_OB"] = str(ob)
    return dict(n=n, L=L, n_out=n_out, groups=G, local=local, first=first, outs=outs, env=env, want_ob=want_ob, ragged=ragged)


def chosen_groups(p):
    """global indices of the first and the last group of every size"""
    return [int(f) + i for f, g in zip(p["first"], p["groups"]) for i in (0, len(g) - 1)]


def one_entry_allocations(p):
    """(24, L): every value of VALUES as the only entry, in each chosen group"""
    M = np.zeros((len(chosen_groups(p)) * len(VALUES), p["L"]))
    for r, (gi, x) in enumerate((gi, x) for gi in chosen_groups(p) for x in VALUES):
        M[r, gi] = x
    return M


def expected(p, m):
    """per output (touched above 1e-6 per model, touched at all per model, max|m| >= 0.05, status) of allocation vector m: the
    flags of k_fold_to_record and the status solve_wave derives from them (no singular system among the cases used here)"""
    out = []
    for gl in p["local"]:
        am = np.zeros(p["n"])
        for f, g in zip(p["first"], gl):
            for j in range(g.shape[1]):
                np.maximum.at(am, g[:, j], np.abs(m[f:f + len(g)]))      # (a local list is a prefix of the global one of its size)
        f1, f2, big = am > 1.0e-6, am > 0.0, bool(am.max() >= 0.05)
        st = INF if not big else (NO_MODEL0 if not f1[0] else OK)
        out.append((f1, f2, big, st))
    return out


@pytest.mark.parametrize("name", NAMES)
def test_expectation_is_self_consistent(name):
    """CPU: the restatement against what a single entry x in group S must give, written out by hand -- flags on S only, above
    1e-6 for 2e-6 / 0.06 / 0.04, large for 0.06 only; INF unless large, else OK exactly when model 0 is in S; an output that
    does not hold the group sees nothing.  The chosen groups hold a singleton, model 0 and a group of the largest size, and all
    three statuses occur.  The ragged plan, and only that one, has unequal workgroups per output."""
    p = problem(name)
    flat = [tuple(int(x) for x in r) for g in p["groups"] for r in g]
    chosen = chosen_groups(p)
    assert len(chosen) == 6 and len(set(chosen)) == 6
    assert any(len(flat[gi]) == 1 for gi in chosen) and any(len(flat[gi]) == 3 for gi in chosen)
    assert sum(0 in flat[gi] for gi in chosen) == 3
    M = one_entry_allocations(p)
    assert M.shape == (24, p["L"]) and ((M != 0).sum(axis=1) == 1).all()
    seen = set()
    for r, (gi, x) in enumerate((gi, x) for gi in chosen for x in VALUES):
        for o, (f1, f2, big, st) in enumerate(expected(p, M[r])):
            held = len(flat[gi]) <= 2 or not p["ragged"] or o == 0
            S = set(flat[gi]) if held else set()
            assert set(np.flatnonzero(f2)) == S
            assert set(np.flatnonzero(f1)) == (S if x > 1.0e-6 else set())
            assert big == (held and x == 0.06)
            assert st == (INF if not big else (OK if 0 in S else NO_MODEL0))
            seen.add(st)
    assert seen == {OK, INF, NO_MODEL0}
    lay = sgc.layout(dict(n=p["n"], n_out=p["n_out"], local=p["local"], groups=p["groups"]))
    assert (lay["bpo"] == 0) == p["ragged"], lay
    assert (lay["nt"] > p["n"]) == (p["n"] == 6)


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def _same(a, b, what):
    a, b = a.cpu().numpy() if hasattr(a, "cpu") else a, b.cpu().numpy() if hasattr(b, "cpu") else b
    assert a.shape == b.shape and a.dtype == b.dtype, what
    assert np.array_equal(_bits(a), _bits(b)), what


@pytest.fixture(params=NAMES)
def case(request, monkeypatch):
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    from bluest_amd.plan import Plan
    p = problem(request.param)
    for k in ENV_KEYS:
        monkeypatch.delenv(k, raising=False)
    for k, v in p["env"].items():
        monkeypatch.setenv(k, v)
    plan = Plan(p["n"], p["L"], p["outs"], max_candidates=24)
    for nc in (1, 3, 24):
        cfg = plan.launch_config(nc)
        assert cfg["phi_ob"] == p["want_ob"] and cfg["path"] == (1 if nc == 1 else 0), cfg      # (one candidate: the fused k_solve_grad)
        assert cfg["cols16"] == (0 if "BLUEST_COLS32" in p["env"] else 1) and cfg["iters"] == 1, cfg
    return p, plan


@pytest.mark.gpu
def test_paths_agree(case):
    import torch
    from bluest_amd.plan import _stream
    from bluest_amd._lib import check
    p, plan = case
    L, n_out = p["L"], p["n_out"]
    rng = np.random.RandomState(9100 + n_out)
    M = 0.5 + rng.rand(3, L)
    M[1] *= rng.rand(L) < 0.7
    M[1, :p["n"]] = 0.75                                   # the singletons stay sampled
    singles = []
    for c in range(3):
        v, g, st = plan.eval(M[c])
        singles.append((v.cpu().numpy(), g.cpu().numpy(), st.cpu().numpy()))
        assert not singles[-1][2].any(), singles[-1][2]
        # split path and record-fed fused kernel
        rec = plan.phi(M[c])
        v2, vv, st2 = plan.solve(rec)
        g2 = plan.grad(vv, st2)
        _same(v2, singles[-1][0], "split V %d" % c); _same(g2, singles[-1][1], "split grad %d" % c); _same(st2, singles[-1][2], "split status %d" % c)
        v3, g3, st3 = plan.solve_grad(rec)
        _same(v3, singles[-1][0], "record V %d" % c); _same(g3, singles[-1][1], "record grad %d" % c); _same(st3, singles[-1][2], "record status %d" % c)
    # the batch, rows PAD doubles apart, the padding poisoned
    buf = np.full((3, L + PAD), np.nan)
    buf[:, :L] = M
    d = torch.from_numpy(buf).to(plan.device)
    var = torch.empty((3, n_out), dtype=torch.float64, device=plan.device)
    grad = torch.empty((3, plan.grad_len), dtype=torch.float64, device=plan.device)
    status = torch.empty((3, n_out), dtype=torch.int32, device=plan.device)
    with torch.cuda.device(plan.device):
        check(plan.lib.bluest_plan_eval(plan._h, d.data_ptr(), 3, L + PAD, 0.0, var.data_ptr(), grad.data_ptr(), grad.stride(0),
                                        status.data_ptr(), _stream()))
    back = d.cpu().numpy()
    assert np.isnan(back[:, L:]).all() and np.array_equal(_bits(back[:, :L]), _bits(M))
    for c in range(3):
        _same(var[c:c + 1], singles[c][0], "batch V %d" % c)
        _same(grad[c:c + 1], singles[c][1], "batch grad %d" % c)
        _same(status[c:c + 1], singles[c][2], "batch status %d" % c)


@pytest.mark.gpu
def test_one_entry_flags_and_status(case):
    p, plan = case
    N, n_out = p["n"], p["n_out"]
    M = one_entry_allocations(p)
    want = [expected(p, m) for m in M]
    rec = plan.phi(M).cpu().numpy()
    assert rec.shape == (len(M), n_out, N * N + 2 * N + 1)
    sts = []
    for r, m in enumerate(M):
        one = plan.phi(m).cpu().numpy()
        assert np.array_equal(_bits(one[0]), _bits(rec[r])), r
        sts.append(plan.eval(m)[2])
    sts = np.concatenate([s.cpu().numpy() for s in sts])
    st_batch = plan.eval(M)[2].cpu().numpy()
    for r in range(len(M)):
        for o, (f1, f2, big, st) in enumerate(want[r]):
            what = (r, o, float(M[r].max()))
            assert np.array_equal(rec[r, o, N * N:N * N + N], f1.astype(np.float64)), what
            assert np.array_equal(rec[r, o, N * N + N:N * N + 2 * N], f2.astype(np.float64)), what
            assert rec[r, o, N * N + 2 * N] == float(big), what
            assert sts[r, o] == st and st_batch[r, o] == st, what + (int(sts[r, o]), int(st_batch[r, o]), st)

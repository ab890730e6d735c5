"""
CPU tests of the numpy restatement of the MLMC subset search (tests/mlmc_ref.py) and of the case table (tests/mlmc_cases.py):
the restatement, driven through the host finishing of setup_mlmc, reproduces every reference fixture tests/golden/mlmc_*.npz
(tools/gen_golden_mlmc.py); the fixtures and the table cover what they are meant to cover.
"""
import glob
import os

import numpy as np
import pytest

import mlmc_cases as mc
import mlmc_ref as ref
from conftest import GOLDEN, golden

FIXTURES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "mlmc_*.npz")) if "helpers" not in f)
CASES = mc.all_cases()


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _kwargs(g):
    kw = {"continuous_relaxation": bool(g["continuous_relaxation"])}
    if "budget" in g: kw["budget"] = float(g["budget"][0])
    else: kw["eps"] = [float(e) for e in g["eps"]] if len(g["eps"]) > 1 else float(g["eps"][0])
    return kw


def _solve(g):
    dV = list(g["mlmc_variances"]) if "mlmc_variances" in g else None
    args, idx = ref.inputs_from_covariances(list(g["C"]), g["costs"], dV, **_kwargs(g))
    r = ref.search(**args)
    assert r.rc == 0 and r.status == ref.OK
    return args, idx, r


def test_fixture_list():
    assert len(FIXTURES) == 20


@pytest.mark.parametrize("name", FIXTURES)
def test_restatement_reproduces_the_reference(name):
    g = golden("mlmc_%s.npz" % name)
    args, idx, r = _solve(g)
    d = ref.host_finish(args, idx, r.best_mask, r.best_combo)
    assert d["models"] == g["models"].tolist()
    assert np.asarray(d["samples"]).dtype.kind == g["samples"].dtype.kind
    if g["samples"].dtype.kind == "i": assert np.array_equal(d["samples"], g["samples"])
    else: assert _rel(d["samples"], g["samples"]) < 1e-12
    assert _rel(d["errors"], g["errors"]) < 1e-12 and _rel(d["total_cost"], g["total_cost"]) < 1e-12
    if not g["continuous_relaxation"]:
        assert r.facts["bounds_hold"]                             # LB <= rounded objective <= UB for every group
        r2 = ref.search(full=True, **args)                        # all 2^L combinations: the same first minimum
        assert r2.best_mask == r.best_mask and np.array_equal(r2.best_combo, r.best_combo) and r2.best_obj == r.best_obj


def _one_group(args, mask):
    P = ref._Prob()
    P.nb, P.n_out, P.budget, P.budget_mode = args["nb"], 1, args["budget"], bool(args["flags"] & ref.BUDGET)
    P.w, P.lv, P.eps2 = args["w"], args["lv"], args["eps2"]
    return P, ref._Level(P, ref.members_of([mask], bin(mask).count("1") + 1, P.nb), 0)


def test_helpers_fixture_is_reproduced():
    """attempt_mlmc_setup of the reference on every group of the 5-model problem, in all four modes, against the restatement's
    levels, allocation and rounding of that one group"""
    g = golden("mlmc_helpers_n5.npz")
    seen = set()
    for k in range(int(g["n_attempts"])):
        mode, group = str(g["a%d_mode" % k]), g["a%d_group" % k].tolist()
        kw = {"budget" if "budget" in mode else "eps": float(g["kw_" + mode]), "continuous_relaxation": mode.endswith("cont")}
        args, idx = ref.inputs_from_covariances([g["C"]], g["costs"], **kw)
        assert idx.tolist() == [0, 1, 2, 3, 4]
        P, V = _one_group(args, sum(1 << (p - 1) for p in group[1:]))
        assert _rel(V.v[0], g["a%d_v" % k]) < 1e-15 and _rel(V.c[0], g["a%d_c" % k]) < 1e-15
        if mode.endswith("cont"):
            ok, m = bool(V.finite[0]), V.m
        else:
            fval, _, m = ref._round_output(P, V, 0, False)
            ok = bool(V.finite[0] and fval[0] < ref.INF)
        assert ok == bool(g["a%d_ok" % k])
        if not ok: continue
        want = g["a%d_samples" % k]
        if want.dtype.kind == "i": assert np.array_equal(m[0], want)
        else: assert _rel(m[0], want) < 1e-12
        assert _rel(np.sqrt(V.variance(m))[0], g["a%d_error" % k]) < 1e-12 and _rel(V.cost(m)[0], g["a%d_cost" % k]) < 1e-12
        seen.add((mode, len(group)))
    assert {m for m, _ in seen} == set(mc.MODES) and {L for _, L in seen} == {1, 2, 3, 4, 5}


def test_fixture_conditions():
    """what the fixtures were chosen for (tools/gen_golden_mlmc.py)"""
    G = {name: golden("mlmc_%s.npz" % name) for name in FIXTURES}
    assert max(len(g["models"]) for g in G.values()) >= 4
    assert {len(G["n%d_eps" % n]["models"]) for n in (6, 8, 10)} == {3, 4, 5}
    for name in ("three_out_eps", "three_out_budget", "unsorted_eps", "unsorted_budget"):     # per-output roundings differ
        outs = [G[name]["out%d_samples" % n] for n in range(len(G[name]["C"]))]
        assert all(not np.array_equal(a, b) for a, b in zip(outs[:-1], outs[1:]))
    plain = G["three_out_eps"]["models"].tolist()
    assert plain == [0, 1, 3, 5]
    for name in ("three_out_eps_dV", "three_out_eps_cut13", "three_out_eps_cut01"):
        assert np.array_equal(G[name]["costs"], G["three_out_eps"]["costs"]) and np.array_equal(G[name]["eps"], G["three_out_eps"]["eps"])
        assert G[name]["models"].tolist() == [0, 2, 3, 5] != plain
    assert G["three_out_eps_dV_inf"]["models"].tolist() == plain             # an entry that is not finite is not used
    assert np.isinf(G["three_out_eps_cut01"]["C"][1][0, 1]) and np.isfinite(G["three_out_eps_cut01"]["C"][0][0, 1])
    for name in ("unsorted_eps", "unsorted_budget"):
        w, models = G[name]["costs"], G[name]["models"].tolist()
        assert (w > w[0]).sum() == 1 and np.flatnonzero(w > w[0])[0] not in models
        assert not np.array_equal(np.argsort(w)[::-1], np.arange(len(w)))
        assert models != sorted(models) or w[2] < w[4]                     # costs out of index order among the candidates


# ---- the case table -------------------------------------------------------------------------------------------------------
def _by_group(group):
    return [c for c in CASES if c["group"] == group]


def test_table_names_are_unique():
    names = [c["name"] for c in CASES]
    assert len(names) == len(set(names))


def test_table_base_and_veto():
    base = _by_group("base")
    assert len(base) == 4 * 3 * 4
    assert {(c["args"]["nb"], c["args"]["n_out"], c["args"]["flags"]) for c in base} == \
        {(nb, no, f) for nb in (0, 1, 2, 7) for no in (1, 3, 64) for f in mc.MODES.values()}
    for c in base:
        r = mc.reference(c)
        assert r.rc == 0 and r.status == ref.OK
    assert max(mc.reference(c).facts["winner_size"] for c in base) >= 4
    for c in _by_group("veto"):
        plain = next(p for p in CASES if p["name"] == c["plain"])
        rp, rv = mc.reference(plain), mc.reference(c)
        p, q = c["pair"]
        assert p == 0 and (rp.best_mask & -rp.best_mask).bit_length() == q      # the plain winner uses the pair
        lv = c["args"]["lv"]
        assert np.isnan(lv[1, p, q]) and np.isfinite(lv[0, p, q]) and np.isfinite(lv[2, p, q])
        assert rv.status == ref.OK and rv.best_mask != rp.best_mask
        assert rv.facts["feasible"] < rp.facts["feasible"]


def test_table_graph():
    for c in _by_group("graph"):
        r, a = mc.reference(c), c["args"]
        assert a["nb"] in (21, 30) and r.status == ref.OK
        assert 100 <= r.facts["groups"] <= 999 and r.facts["largest"] <= 7
        assert r.facts["highest_bit"] >= 20
    assert {c["args"]["nb"] for c in _by_group("graph")} == {21, 30}


def test_table_window():
    for c in _by_group("window"):
        r = mc.reference(c)
        assert c["args"]["nb"] == 17 and r.facts["groups"] == 1 << 17 and r.status == ref.OK
        assert r.facts["candidates"] > ref.CAND_CAP                     # the first window cannot hold them: the loop bisects
        assert r.facts["most_sharing_one_lb"] <= ref.CAND_CAP           # and can always advance
        assert r.facts["bounds_hold"]
    assert {c["args"]["flags"] for c in _by_group("window")} == {mc.EPS, mc.BUDGET}


def test_table_ties():
    seen = set()
    for c in _by_group("tie"):
        r = mc.reference(c)
        assert r.status == ref.OK and r.facts["tied_masks"]
        size = bin(r.best_mask).count("1")
        others = {bin(m).count("1") for m in r.facts["tied_masks"]}
        if c["tie"] == "same":
            assert size in others
            peer = next(m for m in r.facts["tied_masks"] if bin(m).count("1") == size)
            d = r.best_mask ^ peer
            assert not r.best_mask & (d & -d)                            # the winner removed the lower position
        else:
            assert others == {size - 1}                                  # the larger group comes first
        seen.add((c["tie"], c["args"]["flags"]))
    assert seen == {(t, f) for t in ("same", "sizes") for f in mc.MODES.values()}


def test_table_status_and_args():
    S = {c["name"]: c for c in _by_group("status")}
    r = mc.reference(S["none_budget_below_w0"])
    assert r.status == ref.NONE and r.best_mask == 0xffffffff and r.best_obj == ref.INF
    assert S["none_budget_below_w0"]["args"]["budget"] < S["none_budget_below_w0"]["args"]["w"][0]
    for name in ("too_big", "too_big_budget"):
        r = mc.reference(S[name])
        assert S[name]["args"]["nb"] == 25 and r.status == ref.TOO_BIG and r.best_mask is None
    r = mc.reference(S["too_big_input_continuous"])
    assert r.status == ref.OK and np.array_equal(S["too_big_input_continuous"]["args"]["lv"], S["too_big"]["args"]["lv"], equal_nan=True)
    v = mc.valid_small()
    assert mc.reference(v).status == ref.OK
    for name, change in mc.arg_cases():
        change = dict(change)
        given = change.pop("outputs_given", True)
        assert ref.search(outputs_given=given, **dict(v["args"], **change)).rc == ref.ERR_ARG, name


def test_order_key_is_the_reference_enumeration():
    """blue_models.py:664-670 for 5 models, complete graph"""
    from itertools import combinations
    want = [0]
    for i in range(4):
        for remove in combinations(range(1, 5), i):
            want.append(sum(1 << (p - 1) for p in range(1, 5) if p not in remove))
    got = sorted(ref.enumerate_groups(4, mc.complete(4)), key=lambda m: ref.order_key(m, 4))
    assert got == want

"""
CPU tests of the MFMC subset-search reference (oracle/mfmc_ref.py) and of the case table the GPU tests run
(tests/mfmc_cases.py): the reference reproduces the reference project's fixtures and the exhaustive restatement of
test_gpu_mfmc.py, its rounding shortcut equals the full 2^L enumeration, every case of the table is decided by margins that
float64 rounding cannot reach, and the table holds a case of every path it is meant to drive.
"""
import numpy as np
import pytest

import mfmc_cases as mc
from conftest import golden
from oracle import mfmc_ref as ref
from test_gpu_mfmc import CASES as FIXTURES, _exhaustive, _kwargs, _multi, _rel

MARGIN = 1e-9           # the kernel's own LB_MARGIN_MIN; accumulated rounding is about 8 L eps ~ 1e-14, seven orders below
TABLE = mc.all_cases()


def _same(a, b):
    assert (a.rc, a.status, a.best_mask) == (b.rc, b.status, b.best_mask)
    assert np.array_equal(a.best_combo, b.best_combo) and a.best_obj == b.best_obj


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_reproduces_fixture(name):
    g = golden("mfmc_%s.npz" % name)
    args, local = ref.inputs_from_covariances(g["C"], g["costs"], **_kwargs(g))
    r = ref.search(**args)
    assert r.rc == ref.RC_OK and r.status == ref.OK
    models, samples = ref.host_samples(args, local, r.best_mask, r.best_combo)
    assert np.array_equal(models, g["models"])
    assert samples.dtype.kind == g["samples"].dtype.kind
    if samples.dtype.kind == "i":
        assert np.array_equal(samples, g["samples"])
    else:
        assert _rel(samples, g["samples"]) < 1e-12
    _same(r, ref.search(full=True, **args))                      # the rounding shortcut against all 2^L combinations


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("mode", ["eps", "budget", "eps_cont", "budget_cont"])
def test_reference_agrees_with_exhaustive_n16(mode, n_out):
    Cs, w = _multi(16, n_out, 7)
    kw = dict(budget=3000 * w[0]) if mode.startswith("budget") else dict(eps=[0.003 * np.sqrt(C[0, 0]) for C in Cs])
    kw["continuous_relaxation"] = mode.endswith("cont")
    args, local = ref.inputs_from_covariances(Cs, w, **kw)
    r = ref.search(**args)
    models, samples = ref.host_samples(args, local, r.best_mask, r.best_combo)
    cl, want, _ = _exhaustive(Cs, w, **kw)
    assert models == [int(j) for j in cl]
    if want.dtype.kind == "i":
        assert np.array_equal(samples, want)
    else:
        assert _rel(samples, want) < 1e-12
    if not kw["continuous_relaxation"]:
        _same(r, ref.search(full=True, **args))


def test_reference_agrees_with_library_mirrors():
    """one clique at a time against bluest_amd.misc (the numpy mirrors setup_mfmc post-processes with)"""
    from bluest_amd import misc
    for c in TABLE:
        r = mc.reference(c)
        a = c["args"]
        if c["group"] != "base" or r.status != ref.OK or a["n_out"] > 3 or c.get("orders_differ"): continue
        cl = np.array([0] + [b + 1 for b in range(a["nb"]) if (r.best_mask >> b) & 1])
        objs = []
        for n in range(a["n_out"]):
            kw = dict(budget=a["budget"]) if a["flags"] & ref.BUDGET else dict(eps=float(np.sqrt(a["eps2"][n])))
            ok, d = misc.attempt_mfmc_setup(a["s"][n][cl], a["rho"][n][cl], a["w"][cl], continuous_relaxation=bool(a["flags"] & 2),
                                            small_budget=bool(a["flags"] & 4), **kw)
            assert ok
            objs.append(d)
        if a["flags"] & ref.BUDGET:
            assert abs(max(d["error"] for d in objs) / r.best_obj - 1) < 1e-12
        else:
            m = np.max([d["samples"] for d in objs], axis=0)
            assert abs(m @ a["w"][cl][misc.mfmc_order(a["rho"][0][cl])] / r.best_obj - 1) < 1e-12


@pytest.mark.parametrize("name", [c["name"] for c in TABLE])
def test_case_is_sound(name):
    """every decision on the way is further from flipping than rounding can reach; the best clique is best by more than that,
    or ties exactly on purpose"""
    c = next(c for c in TABLE if c["name"] == name)
    r = mc.reference(c)
    F = r.facts
    assert r.rc == c["rc"]
    if r.rc:
        # BLUEST_ERR_STATE is decided by how many cliques share the lower bound zero exactly, a count; no allocation is rounded
        assert F["rounded"] == 0 and F["margins"]["cost_ratio_vs_rho_ratio"] > MARGIN
        return
    for what, margin in F["margins"].items():
        assert margin > MARGIN, (what, margin)
    assert F["m_exact_integers"] == 0
    if r.status != ref.OK: return
    if c["tie"]:
        assert F["runner_up_gap"] == 0.0 and F["ties"] == 1
        other = F["tied_masks"][0]
        if "dup" in c:                                            # the two masks differ in the copy and its original alone
            src, dup = c["dup"]
            assert r.best_mask ^ other == (1 << src) | (1 << dup) and (r.best_mask >> src) & 1
            a = c["args"]
            assert all(np.array_equal(x[..., src + 1], x[..., dup + 1]) for x in (a["w"], a["s"], a["rho"]))
        else:                                                     # the ghost model: the larger clique loses
            assert other == r.best_mask | (1 << c["ghost"])
    else:
        assert F["runner_up_gap"] > MARGIN and F["ties"] == 0


def _facts(group=None):
    return [(c, mc.reference(c)) for c in TABLE if group is None or c["group"] == group]


def test_table_covers_the_paths():
    """a case removed from the table breaks one of these"""
    ok = [(c, r) for c, r in _facts() if r.rc == 0 and r.status == ref.OK]
    integer = [(c, r) for c, r in ok if "candidates" in r.facts]
    # windows: more than CAND_CAP candidates, eps mode, 1 and 2 outputs; the winner outside the first bisected window
    for n_out in (1, 2):
        hits = [r for c, r in integer if c["args"]["n_out"] == n_out and not c["args"]["flags"] & ref.BUDGET
                and r.facts["candidates"] > ref.CAND_CAP]
        assert hits, n_out
        assert all(r.facts["windows"][0][3] > 0 and r.facts["winner_window"] > 0 for r in hits)
    assert any(not r.facts["winner_is_min_ub"] for c, r in integer)
    assert any(any(0 < k < r.facts["winner_all_ones"] for k in r.facts["winner_combo"]) for c, r in integer)
    # rounding: a winner of at least 9 models (a lane of k_mfmc_round sees more than one combination) with a clamped
    # position at bound entry j >= 8, so that keeping a lane's last minimum instead of its first changes best_combo
    assert any(r.facts["winner_size"] >= 9 and any(j >= 8 for cl in r.facts["winner_clamped_entries"] for j in cl)
               and r.facts["winner_last_minimum_combo"] != r.facts["winner_combo"] for c, r in integer)
    wide = [(c, r) for c, r in ok if c["args"]["nb"] >= 21]
    assert any(r.facts["highest_bit"] == 29 for c, r in wide) and any(20 <= r.facts["highest_bit"] < 29 for c, r in wide)
    # ties: the masks meet in one wave, in two waves of a block, in two blocks, in two grid-stride iterations (4096 blocks of
    # 256 masks per iteration); in the exact modes and in the integer mode; and once between cliques of different sizes
    where = set()
    for c, r in ok:
        if not c["tie"]: continue
        a, b = r.best_mask, r.facts["tied_masks"][0]
        assert a < b or bin(a).count("1") < bin(b).count("1")
        integer_mode = "candidates" in r.facts
        if bin(a).count("1") != bin(b).count("1"): where.add(("sizes", integer_mode))
        elif a >> 20 != b >> 20: where.add(("iteration", integer_mode))
        elif a >> 8 != b >> 8: where.add(("block", integer_mode))
        elif a >> 6 != b >> 6: where.add(("wave", integer_mode))
        else: where.add(("lane", integer_mode))
    assert where == {(k, i) for k in ("sizes", "iteration", "block", "wave", "lane") for i in (False, True)}
    # small_budget: the full 6-model clique pins 0, 1, ..., 5 leading models
    pins = set()
    for c, r in _facts("small_budget"): pins |= {p for L, p in r.facts["pins"] if L == 6}
    assert pins == set(range(6))
    statuses = {r.status for c, r in _facts() if r.rc == 0}
    assert statuses == {ref.OK, ref.NONE, ref.TOO_BIG}
    assert any(r.status == ref.NONE and c["args"]["flags"] == mc.SMALL for c, r in _facts())
    assert any(r.status == ref.NONE and c["args"]["flags"] == mc.BUDGET for c, r in _facts())
    assert any(r.rc == ref.ERR_STATE for c, r in _facts())
    # base: all five modes at n_out 1, 3, 64 and nb 0, 1, 2, 7; different orders; one output's veto
    seen = {(c["args"]["flags"], c["args"]["n_out"], c["args"]["nb"]) for c, r in _facts("base")}
    assert {(f, n, b) for f in mc.MODES.values() for n in (1, 3, 64) for b in (0, 1, 2, 7)} <= seen
    assert any(not np.array_equal(c["args"]["perm"][0], c["args"]["perm"][1]) for c, r in _facts("base") if c.get("orders_differ"))
    for c, r in _facts("base"):
        if "veto_output" not in c: continue
        a = dict(c["args"])
        keep = [n for n in range(a["n_out"]) if n != c["veto_output"]]
        a.update(n_out=len(keep), s=a["s"][keep], rho=a["rho"][keep], perm=a["perm"][keep],
                 eps2=None if a["eps2"] is None else a["eps2"][keep], epsm2=None if a["epsm2"] is None else a["epsm2"][keep])
        free = ref.search(**a)
        assert free.best_mask != r.best_mask                     # without that output another clique is best ...
        cl = [0] + [b + 1 for b in range(a["nb"]) if (free.best_mask >> b) & 1]
        P = c["args"]
        rank = np.argsort(P["perm"][c["veto_output"]])
        o = sorted(cl, key=lambda q: rank[q])
        rho = np.concatenate([P["rho"][c["veto_output"]][o], [0.0]])
        w = P["w"][o]
        with np.errstate(divide="ignore"):
            assert not np.all(w[:-1] / w[1:] > (rho[:-2]**2 - rho[1:-1]**2) / (rho[1:-1]**2 - rho[2:]**2))   # ... which it vetoes


def test_err_state_case_is_bounded():
    """|rho_1| = 1: the window loop gives up after MAX_IDLE_SCANS counting scans, long before its halvings run out of doubles"""
    c = next(c for c in TABLE if c["rc"] == ref.ERR_STATE)
    r = mc.reference(c)
    assert r.rc == ref.ERR_STATE and ref.MAX_IDLE_SCANS <= r.facts["scans"] <= ref.MAX_IDLE_SCANS + ref.MAX_HALVINGS + 1
    assert all(n == 0 for _, _, n, _ in r.facts["windows"])       # every window so far came out empty

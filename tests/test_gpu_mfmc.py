"""
GPU tests of the MFMC and plain Monte Carlo estimators (BLUEProblem.setup_mfmc / solve_mfmc / compute_mfmc_data / solve_mc;
reference bluest/blue_models.py:773-930) and of the model-subset search kernel (csrc/mfmc.hip), against reference fixtures
(tools/gen_golden_mfmc.py) and an exhaustive numpy restatement.
"""
import time
from itertools import combinations

import numpy as np
import pytest

from conftest import golden

pytestmark = pytest.mark.gpu

CASES = ["tutorial_eps", "tutorial_budget", "tutorial_small_budget", "n8_eps", "n8_eps_cont", "n10_budget", "n10_budget_cont",
         "graph_eps", "graph_budget", "three_out_eps", "three_out_budget", "multi_out_eps", "multi_out_budget", "only_zero"]


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _problem(C, w, **kw):
    from bluest_amd import BLUEProblem
    return BLUEProblem(len(w), C=list(C), costs=w, n_outputs=len(C), verbose=False, **kw)


def _kwargs(g):
    kw = {"continuous_relaxation": bool(g["continuous_relaxation"]), "small_budget": bool(g["small_budget"])}
    if "budget" in g: kw["budget"] = float(g["budget"][0])
    else: kw["eps"] = [float(e) for e in g["eps"]] if len(g["eps"]) > 1 else float(g["eps"][0])
    return kw


@pytest.mark.parametrize("name", CASES)
def test_setup_mfmc_matches_reference(name):
    g = golden("mfmc_%s.npz" % name)
    P = _problem(g["C"], g["costs"])
    d = P.setup_mfmc(**_kwargs(g))
    assert np.array_equal(np.array(d["models"]), g["models"])
    s = np.asarray(d["samples"])
    assert s.dtype.kind == g["samples"].dtype.kind
    if s.dtype.kind == "i":
        assert np.array_equal(s, g["samples"])
    else:
        assert _rel(s, g["samples"]) < 1e-12
    assert _rel(d["errors"], g["errors"]) < 1e-12
    assert _rel(d["total_cost"], g["total_cost"]) < 1e-12
    assert _rel(np.concatenate(d["alphas"]), g["alphas"]) < 1e-12


def test_compute_mfmc_data_and_errors():
    from bluest_amd import BLUESTError  # noqa: F401
    g = golden("mfmc_graph_eps.npz")
    P = _problem(g["C"], g["costs"])
    d = P.compute_mfmc_data(list(g["models"]), g["samples"])
    assert _rel(d["errors"], g["cd_errors"]) < 1e-12 and _rel(d["total_cost"], g["cd_total_cost"]) < 1e-12
    with pytest.raises(ValueError, match="not a clique"):
        P.compute_mfmc_data([0, 2, 4], [10, 20, 30])                  # 2-4 never coupled
    with pytest.raises(ValueError, match="model 0"):
        P.compute_mfmc_data([2, 0], [10, 20])


def _tutorial():
    from scipy.special import gamma
    from bluest_amd import BLUEProblem
    n_models = 5
    g = golden("mfmc_tutorial_eps.npz")

    def series(x, i):
        ii = np.arange(i + 1)
        return np.sum(x ** ii / gamma(ii + 1))
    rng = np.random.RandomState(1)

    class MyProblem(BLUEProblem):
        def sampler(self, ls):
            Z = rng.randn()
            return [float(Z) for i in range(len(ls))]

        def evaluate(self, ls, samples):
            out = [0 for i in range(len(ls))]
            for i in range(len(ls)):
                if ls[i] == 0: out[i] = np.exp(samples[i])
                elif ls[i] < n_models - 1: out[i] = series(samples[i], n_models - ls[i])
                else: out[i] = np.log(abs(samples[i]))
            return [out]
    return MyProblem(n_models, C=g["C"][0], costs=g["costs"], verbose=False), g


def test_solve_mc_and_solve_mfmc_tutorial():
    P, g = _tutorial()
    eps = 0.03 * np.sqrt(g["C"][0][0, 0])
    mu, errs, cost = P.solve_mc(eps=eps)
    assert abs(mu[0] - np.exp(0.5)) < 6 * errs[0] and errs[0] <= eps and cost == np.ceil(g["C"][0][0, 0] / eps**2) * 32
    d = P.setup_mfmc(eps=eps)
    mu, errs, cost = P.solve_mfmc(eps=eps, mfmc_data=d)
    assert abs(mu[0] - np.exp(0.5)) < 6 * errs[0]
    assert np.array_equal(errs, d["errors"]) and cost == d["total_cost"] and max(errs) <= eps * (1 + 1e-12)
    mu, errs, cost = P.solve_mc(budget=200 * 32)
    assert abs(mu[0] - np.exp(0.5)) < 6 * errs[0] and cost == 200 * 32


def test_multi_output_fixtures_have_distinct_outputs():
    """the multi_out fixtures exercise the per-output search: the outputs' rounded samples on the chosen clique differ, and in
    budget mode the per-model maximum takes entries from more than one output"""
    for name in ("multi_out_eps", "multi_out_budget"):
        g = golden("mfmc_%s.npz" % name)
        outs = [g["out%d_samples" % n] for n in range(3)]
        assert not np.array_equal(outs[0], outs[1]) and not np.array_equal(outs[1], outs[2])
        assert len(set(np.round(g["errors"], 12))) == 3
    outs = np.vstack([golden("mfmc_multi_out_budget.npz")["out%d_samples" % n] for n in range(3)])
    assert len(set(np.argmax(outs, axis=0).tolist())) > 1


def _multi(n, n_out, seed):
    """output o: X_j = a_j^(1 + 0.3 o) X_0 + noise -- values differ per output, |rho| order is the same"""
    rng = np.random.RandomState(seed)
    a = np.concatenate([[1.0], np.clip(1 - 0.02 * np.cumsum(rng.uniform(0.2, 1.0, n - 1)), 0.05, 1.0)])
    w = 10.0 ** (3 - 4.0 * np.arange(n) / (n - 1)) * rng.uniform(0.9, 1.1, n)
    w[0] = w.max() * 1.01
    Cs = []
    for o in range(n_out):
        ao = a ** (1 + 0.3 * o)
        R = np.outer(ao, ao)
        np.fill_diagonal(R, 1.0)
        Cs.append(R * np.outer(*(2 * [rng.uniform(0.5, 2.0, n)])))
    return Cs, w


def _mfmc_clique(s, rho, w, budget, eps, continuous):
    """misc.py:78-130 and 141-175, 384-413 restated here for one clique and one output (models in |rho| order, ties by stable
    sort): None if infeasible, else (order, samples, variance of rows)"""
    o = np.argsort(np.abs(rho), kind="stable")[::-1]
    s, w, r = s[o], w[o], np.concatenate([rho[o], [0.0]])
    with np.errstate(divide="ignore", invalid="ignore"):
        if not np.all(w[:-1] / w[1:] > (r[:-2]**2 - r[1:-1]**2) / (r[1:-1]**2 - r[2:]**2)):
            return None
    q = np.sqrt(w[0] / w * (r[:-1]**2 - r[1:]**2) / (1 - r[1]**2))
    m1 = budget / (w @ q) if budget is not None else eps**-2 * (w @ q) * (s[0]**2 / w[0]) * (1 - r[1]**2)
    m = np.maximum(np.concatenate([[m1], m1 * q[1:]]), 1)
    al = r[1:-1] * s[0] / s[1:]
    coef = al**2 * s[1:]**2 - 2 * al * r[1:-1] * s[0] * s[1:]

    def var(ms):
        ms = np.atleast_2d(ms)
        acc = 0
        for i in range(1, ms.shape[1]):
            acc = acc + (1 / ms[:, i - 1] - 1 / ms[:, i]) * coef[i - 1]
        return s[0]**2 / ms[:, 0] + acc
    if continuous:
        return o, m, var
    L = len(m)
    srt = np.argsort(m, kind="stable")
    lb, ub = np.floor(m).astype(int)[srt], np.ceil(m).astype(int)[srt]
    pos = srt[np.argsort(lb, kind="stable")[::-1]]            # get_feasible_integer_bounds order
    bits = (np.arange(2**L)[:, None] >> np.arange(L)[None, :]) & 1   # unpackbits
    ms = np.empty((2**L, L), dtype=np.int64)
    ms[:, pos] = np.where(bits == 1, np.ceil(m).astype(int)[pos], np.floor(m).astype(int)[pos])
    ok = (ms[:, 0] >= 1) & np.all(ms[:, :-1] <= ms[:, 1:], axis=1)
    v = var(ms)
    f = np.where(ok & (ms @ w <= budget), v, np.inf) if budget is not None else np.where(ok & (v <= eps**2), ms @ w, np.inf)
    c = int(np.argmin(f))
    return (o, ms[c], var) if np.isfinite(f[c]) else None


def _exhaustive(Cs, w, budget=None, eps=None, continuous_relaxation=False):
    """blue_models.py:797-865 restated: every clique through model 0 of a complete graph, size then lexicographic order, strict
    '<'; eps mode: cost of the per-model maximum over outputs, budget mode: the largest error; then the budget floor correction"""
    n = len(w)
    best, best_val = None, np.inf
    for size in range(1, n + 1):
        for sub in combinations(range(1, n), size - 1):
            cl = np.array((0,) + sub)
            res = []
            for k, C in enumerate(Cs):
                s = np.sqrt(np.diag(C))
                got = _mfmc_clique(s[cl], (C / np.outer(s, s))[0][cl], w[cl], budget, None if eps is None else eps[k],
                                   continuous_relaxation)
                if got is None: break
                res.append(got)
            if len(res) < len(Cs): continue
            order = res[0][0]
            assert all(np.array_equal(r[0], order) for r in res)
            if budget is not None:
                val = max(float(np.sqrt(var(m)[0])) for _, m, var in res)
            else:
                val = np.max(np.vstack([m for _, m, _ in res]), axis=0) @ w[cl][order]
            if val < best_val:
                best, best_val = (cl[order], res), val
    cl, res = best
    samples = np.max(np.vstack([m for _, m, _ in res]), axis=0)
    if budget is not None:
        wm = w[cl]
        samples = np.floor(samples - (max(samples @ wm - budget, 0) / (wm @ wm)) * wm).astype(np.int64)
        samples[0] = max(samples[0], 1)
    return cl, samples, [float(np.sqrt(var(samples)[0])) for _, _, var in res]


@pytest.mark.parametrize("n_out", [1, 2])
@pytest.mark.parametrize("mode", ["eps", "budget", "eps_cont", "budget_cont"])
def test_n16_complete_graph_against_exhaustive(mode, n_out):
    Cs, w = _multi(16, n_out, 7)
    kw = dict(budget=3000 * w[0]) if mode.startswith("budget") else dict(eps=[0.003 * np.sqrt(C[0, 0]) for C in Cs])
    kw["continuous_relaxation"] = mode.endswith("cont")
    P = _problem(Cs, w)
    t0 = time.perf_counter()
    d = P.setup_mfmc(**kw)
    t_gpu = time.perf_counter() - t0
    cl, samples, errs = _exhaustive(Cs, w, **kw)
    assert list(d["models"]) == [int(j) for j in cl]
    assert np.asarray(d["samples"]).dtype.kind == samples.dtype.kind
    if samples.dtype.kind == "i":
        assert np.array_equal(d["samples"], samples)
    else:
        assert _rel(d["samples"], samples) < 1e-12
    assert _rel(d["errors"], errs) < 1e-12
    print("n=16 %s, %d outputs: %d models, GPU search %.3f s" % (mode, n_out, len(cl), t_gpu))


def test_outputs_with_different_nesting_order_are_refused():
    """the best clique holds models 1 and 2, which output 0 sorts (1, 2) and output 1 sorts (2, 1) by |rho|: one MFMC estimator
    cannot nest both, so setup_mfmc refuses instead of returning errors that solve_mfmc would not achieve"""
    from bluest_amd import BLUESTError

    def cov(r, s):
        a = np.array([1.0] + list(r))
        R = np.outer(a, a)
        np.fill_diagonal(R, 1.0)
        return R * np.outer(s, s)
    Cs = [cov([0.99, 0.97], [1, 1, 1]), cov([0.97, 0.99], [1, 1.5, 0.7])]
    w = np.array([1.0, 0.01, 0.008])
    P = _problem(Cs, w)
    for kw in (dict(eps=0.01), dict(budget=100.0)):
        with pytest.raises(BLUESTError, match="differently"):
            P.setup_mfmc(**kw)


def test_limits_raise_reference_exceptions():
    from bluest_amd import BLUESTError
    n = 32
    R = np.full((n, n), 0.5) + 0.5 * np.eye(n)
    with pytest.raises(BLUESTError, match="31 neighbours"):
        _problem([R], np.linspace(1, 0.5, n)).setup_mfmc(eps=0.1)       # model 0 with 31 neighbours
    # 26 models whose full clique is ordering-feasible: |rho| and costs falling fast enough
    n = 26
    a = np.concatenate([[1.0], 0.9999 ** (np.arange(1, n) ** 2)])
    R = np.outer(a, a)
    np.fill_diagonal(R, 1.0)
    w = 10.0 ** (-0.6 * np.arange(n))
    with pytest.raises(ValueError, match="Too many dimensions"):
        _problem([R], w).setup_mfmc(eps=1e-3)


def test_mlmc_still_refused():
    from bluest_amd import BLUESTError
    g = golden("mfmc_tutorial_eps.npz")
    P = _problem(g["C"], g["costs"])
    with pytest.raises(BLUESTError):
        P.setup_mlmc(eps=0.1)
    with pytest.raises(BLUESTError):
        P.setup_mc(eps=0.1)

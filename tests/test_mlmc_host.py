"""
CPU tests of the host layer of the MLMC estimator: the single-group mirrors of bluest_amd.misc against the reference's
attempt_mlmc_setup (tests/golden/mlmc_helpers_n5.npz), MLMCMixin.compute_mlmc_data against the reference fixtures, the
mlmc_variances accessors, and the shape of the public interface (BLUEProblem refuses, the mix-in provides).
"""
import numpy as np
import pytest

from conftest import golden


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _problem(g, **kw):
    from bluest_amd import BLUEProblem
    from bluest_amd.mlmc import MLMCMixin

    class P(MLMCMixin, BLUEProblem):
        pass
    dV = list(g["mlmc_variances"]) if "mlmc_variances" in g else None
    return P(len(g["costs"]), C=list(g["C"]), costs=g["costs"], mlmc_variances=dV, n_outputs=len(g["C"]), verbose=False, **kw)


def test_single_group_mirrors_match_the_reference():
    from bluest_amd import misc
    g = golden("mlmc_helpers_n5.npz")
    dV = np.full((5, 5), np.nan)
    n_ok = 0
    for k in range(int(g["n_attempts"])):
        mode, group = str(g["a%d_mode" % k]), g["a%d_group" % k].tolist()
        v, c = misc.mlmc_levels(g["C"], dV, g["costs"], group)
        assert _rel(v, g["a%d_v" % k]) < 1e-15 and _rel(c, g["a%d_c" % k]) < 1e-15
        kw = {"budget" if "budget" in mode else "eps": float(g["kw_" + mode]), "continuous_relaxation": mode.endswith("cont")}
        ok, d = misc.attempt_mlmc_setup(v, c, **kw)
        assert ok == bool(g["a%d_ok" % k])
        if not ok:
            assert d is None
            continue
        n_ok += 1
        want = g["a%d_samples" % k]
        assert np.asarray(d["samples"]).dtype.kind == want.dtype.kind
        if want.dtype.kind == "i": assert np.array_equal(d["samples"], want)
        else: assert _rel(d["samples"], want) < 1e-12
        assert _rel(d["error"], g["a%d_error" % k]) < 1e-12 and _rel(d["total_cost"], g["a%d_cost" % k]) < 1e-12
        assert _rel(np.sqrt(d["variance"](d["samples"])), d["error"]) == 0.0
    assert n_ok >= 48
    with pytest.raises(ValueError, match="budget or RMSE"):
        misc.attempt_mlmc_setup(np.ones(2), np.ones(2))
    assert misc.attempt_mlmc_setup(np.array([1.0, np.inf]), np.ones(2), eps=0.1) == (False, None)


def test_mlmc_levels_uses_finite_mlmc_variances():
    from bluest_amd import misc
    g = golden("mlmc_three_out_eps_dV.npz")
    C, dV, w = g["C"][0], g["mlmc_variances"][0], g["costs"]
    v, c = misc.mlmc_levels(C, dV, w, [0, 1, 3, 5])
    assert v[1] == dV[1, 3] == 50 * C[1, 1]
    assert v[0] == C[0, 0] + (C[1, 1] - 2 * C[0, 1]) and v[3] == C[5, 5]
    assert np.array_equal(c, [w[0] + w[1], w[1] + w[3], w[3] + w[5], w[5]])
    dV = dV.copy()
    dV[1, 3] = np.inf
    assert misc.mlmc_levels(C, dV, w, [0, 1, 3, 5])[0][1] == C[1, 1] + (C[3, 3] - 2 * C[1, 3])
    v, c = misc.mlmc_levels(C, dV, w, [0])
    assert v.tolist() == [C[0, 0]] and c.tolist() == [w[0]]


@pytest.mark.parametrize("name", ["n10_eps", "three_out_budget", "three_out_eps_dV", "three_out_eps_cut13", "unsorted_eps"])
def test_compute_mlmc_data_matches_the_reference(name, capsys):
    g = golden("mlmc_%s.npz" % name)
    P = _problem(g)
    d = P.compute_mlmc_data(g["models"].tolist(), g["samples"])
    assert _rel(d["errors"], g["cd_errors"]) < 1e-12 and _rel(d["total_cost"], g["cd_total_cost"]) < 1e-12
    assert d["models"] == g["models"].tolist() and np.array_equal(d["samples"], g["samples"])
    warned = "MLMC variances were not provided" in capsys.readouterr().out
    assert warned == ("mlmc_variances" not in g)


def test_compute_mlmc_data_errors():
    g = golden("mlmc_three_out_eps_cut13.npz")
    P = _problem(g)
    with pytest.raises(ValueError, match="not compatible with MLMC"):
        P.compute_mlmc_data([0, 1, 3, 5], [10, 20, 30, 40])           # 1-3 never coupled
    with pytest.raises(ValueError, match="model 0"):
        P.compute_mlmc_data([2, 3], [10, 20])


def test_mlmc_variances_default_and_wrapping():
    from bluest_amd import BLUEProblem
    g = golden("mlmc_three_out_eps_dV.npz")
    P = BLUEProblem(7, C=list(g["C"]), costs=g["costs"], n_outputs=3, verbose=False)
    dV = P.get_mlmc_variances()
    assert len(dV) == 3 and all(d.shape == (7, 7) and np.isnan(d).all() for d in dV)
    assert P.get_mlmc_variance(2) is dV[2]
    one = g["mlmc_variances"][0]
    P = BLUEProblem(7, C=g["C"][0], costs=g["costs"], mlmc_variances=one, verbose=False)
    assert isinstance(P.get_mlmc_variances(), list) and P.get_mlmc_variance() is one
    given = list(g["mlmc_variances"])
    P = BLUEProblem(7, C=list(g["C"]), costs=g["costs"], mlmc_variances=given, n_outputs=3, verbose=False)
    assert P.get_mlmc_variances() is given


def test_the_class_refuses_and_the_mixin_provides():
    from bluest_amd import BLUEProblem, BLUESTError
    from bluest_amd.mlmc import MLMCMixin
    assert BLUEProblem.setup_mlmc is BLUEProblem._out_of_scope and BLUEProblem.solve_mlmc is BLUEProblem._out_of_scope

    class P(MLMCMixin, BLUEProblem):
        pass
    for name in ("setup_mlmc", "solve_mlmc", "compute_mlmc_data"):
        assert getattr(P, name) is getattr(MLMCMixin, name)
    assert P.setup_mc is BLUEProblem._out_of_scope
    g = golden("mlmc_n6_eps.npz")
    with pytest.raises(BLUESTError):
        BLUEProblem(6, C=g["C"][0], costs=g["costs"], verbose=False).setup_mlmc(eps=0.1)
    p = P(6, C=g["C"][0], costs=g["costs"], verbose=False)
    with pytest.raises(ValueError, match="budget or RMSE"):
        p.setup_mlmc()
    with pytest.raises(ValueError, match="budget or RMSE"):
        p.solve_mlmc()


def test_solve_mlmc_refuses_a_level_without_samples():
    from bluest_amd import BLUESTError
    g = golden("mlmc_n6_eps.npz")
    p = _problem(g)
    data = {"models": [0, 2, 4], "samples": np.array([3, 0, 7]), "errors": [0.1], "total_cost": 1.0}
    with pytest.raises(BLUESTError, match="no samples"):
        p.solve_mlmc(eps=0.1, mlmc_data=data)


def test_solve_mlmc_sums_the_level_groups():
    """blue_models.py:759-767 on a model whose levels are known: model j returns j + 1, so every level difference is -gap and the
    estimate is the value of the last model minus the gaps"""
    g = golden("mlmc_n6_eps.npz")
    calls = []

    from bluest_amd import BLUEProblem
    from bluest_amd.mlmc import MLMCMixin

    class P(MLMCMixin, BLUEProblem):
        def sampler(self, ls, N=1): return [0.0 for _ in ls]
        def evaluate(self, ls, samples, N=1): return [[float(l + 1) for l in ls]]

        def _group_sums(self, ls, N):
            calls.append((list(ls), int(N)))
            return BLUEProblem._group_sums(self, ls, N)
    p = P(6, C=g["C"][0], costs=g["costs"], verbose=False)
    data = {"models": [0, 2, 4], "samples": np.array([3, 5, 7]), "errors": [0.25], "total_cost": 12.5}
    mu, errs, cost = p.solve_mlmc(budget=1.0, mlmc_data=data)
    assert calls == [([0, 2], 3), ([2, 4], 5), ([4], 7)]
    assert mu == [1.0] and errs == [0.25] and cost == 12.5

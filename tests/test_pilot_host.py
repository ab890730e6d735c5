"""CPU tests of bluest_amd.pilot: the estimation flow, the sampler call sequence and the model-graph files against what the
reference produced (tests/golden/pilot_*.npz, written by tools/gen_golden_pilot.py), with the GPU sums replaced by the
long-double restatement of tests/pilot_ref.py."""
import os

import numpy as np
import pytest

import pilot_ref
from conftest import GOLDEN
from pilot_ref import cov_bound, scatter, within

CASES = pilot_ref.case_names()
SCALAR_CASES = [c for c in CASES if c != "inner"]


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.pilot import PilotMixin
    return PilotMixin, BLUEProblem


def test_fixtures_are_there():
    assert set(CASES) >= {"none_2out", "partial", "costs_none", "batch1", "one_arg", "projected", "dV_given", "inner"}
    for name in os.listdir(GOLDEN):
        if name.startswith("pilot_"):
            assert os.path.getsize(os.path.join(GOLDEN, name)) < 100 * 1024, name


@pytest.mark.parametrize("name", SCALAR_CASES)
def test_restatement_reproduces_the_reference(name):
    g = pilot_ref.case(name)
    N, values = int(g["N"]), pilot_ref.pilot_values(g)
    assert values.shape == (int(g["n_outputs"]), N, len(g["ls"]))
    sums = pilot_ref.sums_ld(values)
    for mine, ref in zip(sums, (g["fn_sumse"], g["fn_sumsc"], g["fn_sumsd1"], g["fn_sumsd2"])):
        assert np.allclose(np.asarray(mine, dtype=np.float64), ref, rtol=1e-13, atol=1e-13)
    C_hat, dV_hat = pilot_ref.estimates(*sums, N)
    C, dV = pilot_ref.fill(g["C_given"], g["dV_given"], g["ls"], np.asarray(C_hat, dtype=np.float64), np.asarray(dV_hat, dtype=np.float64))
    bc, bd = cov_bound(values, N)
    within(pilot_ref.as_get_covariance(C), g["cov"] if bool(g["skip_projection"]) else g["cov_skip"], scatter(g, bc))
    within(dV, g["dV"], scatter(g, bd))


def test_restatement_reproduces_the_weighted_inner_product_case():
    g = pilot_ref.case("inner")
    w, N = g["vec_weights"].astype(pilot_ref.LD), int(g["N"])
    Y = np.stack(g["blocks"], axis=1).astype(pilot_ref.LD)                   # [n_out, N, L, d]
    inner = lambda a, b: (a * w * b).sum(axis=-1)
    se = Y.sum(axis=1)
    sc = inner(Y[:, :, :, None, :], Y[:, :, None, :, :]).sum(axis=1)
    D = Y[:, :, :, None, :] - Y[:, :, None, :, :]
    upper = np.triu(np.ones((Y.shape[2], Y.shape[2])), 1)
    d1, d2 = D.sum(axis=1) * upper[:, :, None], inner(D, D).sum(axis=1) * upper
    for mine, ref in zip((se, sc, d1, d2), (g["fn_sumse"], g["fn_sumsc"], g["fn_sumsd1"], g["fn_sumsd2"])):
        assert np.allclose(np.asarray(mine, dtype=np.float64), ref, rtol=1e-13, atol=1e-13)
    C_hat = sc / N - inner(se[:, :, None, :], se[:, None, :, :]) / N**2
    dV_hat = d2 / N - inner(d1 / N, d1 / N)
    assert np.allclose(np.asarray(C_hat, dtype=np.float64), g["cov"], rtol=1e-11, atol=1e-12)
    iu = np.triu_indices(Y.shape[2], 1)
    assert np.allclose(np.asarray(dV_hat, dtype=np.float64)[:, iu[0], iu[1]], g["dV"][:, iu[0], iu[1]], rtol=1e-11, atol=1e-12)


@pytest.mark.parametrize("name", CASES)
def test_mixin_reproduces_the_reference(name, monkeypatch):
    from bluest_amd import pilot
    g = pilot_ref.case(name)
    stats_calls = []

    def stats(values, differences=True):
        stats_calls.append(values.shape)
        return pilot_ref.pilot_statistics(values, differences)
    monkeypatch.setattr(pilot, "pilot_statistics", stats)
    P = pilot_ref.replay_class(g, *_classes())(skip_projection=True)
    assert P.calls == g["call_list"]                                   # the reference's sampler calls, in its order
    N = int(g["N"])
    if name == "inner":
        assert stats_calls == []                                        # Python inner products: the sums come from blue_fn
        assert np.allclose(np.array(P.get_covariances()), g["cov"], rtol=1e-12, atol=1e-13, equal_nan=True)
        assert np.allclose(np.array(P.get_mlmc_variances()), g["dV"], rtol=1e-12, atol=1e-13, equal_nan=True)
    else:
        assert stats_calls == [(int(g["n_outputs"]), N, len(g["ls"]))]  # ONE call with all the values
        bc, bd = cov_bound(pilot_ref.pilot_values(g), N)
        within(np.array(P.get_covariances()), g["cov"] if bool(g["skip_projection"]) else g["cov_skip"], scatter(g, bc))
        within(np.array(P.get_mlmc_variances()), g["dV"], scatter(g, bd))
    assert np.array_equal(P.get_costs(), g["costs"])
    assert [list(sg) for sg in P.SG] == pilot_ref.unpadded(g["SG"])


@pytest.mark.parametrize("name", CASES)
def test_blue_fn_returns_the_reference_difference_sums(name):
    g = pilot_ref.case(name)
    P = pilot_ref.replay_class(g, *_classes())
    p = P.__new__(P)                                                    # no constructor: blue_fn alone, on the recorded calls
    p.calls, p.last, k0 = [None] * g["n_cost_calls"], 0, g["n_cost_calls"]
    import bluest_amd
    p.n_outputs = int(g["n_outputs"])
    out = bluest_amd.blue_fn(g["ls"], int(g["N"]), p, sampler=p.sampler, inners=p.get_models_inner_products(), N1=int(g["batch"]),
                             No=int(g["n_outputs"]), verbose=False, compute_mlmc_differences=True)
    assert len(out) == 5 and p.calls[k0:] == g["call_list"][k0:]
    se, sc, _, d1, d2 = out
    L = len(g["ls"])
    zero = np.zeros_like(g["fn_sumse"][0][0])
    assert np.allclose(np.array(se, dtype=np.float64), g["fn_sumse"], rtol=1e-13)
    assert np.allclose(np.array(sc), g["fn_sumsc"], rtol=1e-13)
    assert np.allclose(np.array([[[zero + v for v in row] for row in o] for o in d1], dtype=np.float64), g["fn_sumsd1"], rtol=1e-13, atol=1e-13)
    assert np.allclose(np.array(d2, dtype=np.float64), g["fn_sumsd2"], rtol=1e-13)
    assert all(not np.any(d1[n][i][j]) for n in range(len(d1)) for i in range(L) for j in range(i + 1))


def test_complete_inputs_draw_no_sample(monkeypatch):
    from bluest_amd import pilot
    PilotMixin, BLUEProblem = _classes()
    monkeypatch.setattr(pilot, "pilot_statistics", lambda *a, **k: pytest.fail("nothing is unknown: nothing to compute"))

    class P(PilotMixin, BLUEProblem):
        def sampler(self, ls, N=1): pytest.fail("nothing is unknown: nothing to sample")

    C = np.array([[2.0, 0.5, np.inf], [0.5, 1.0, 0.25], [np.inf, 0.25, 1.5]])
    p = P(3, C=C, costs=[4.0, 2.0, 1.0], verbose=False)
    q = BLUEProblem(3, C=C, costs=[4.0, 2.0, 1.0], verbose=False)
    assert np.array_equal(p.get_covariance(), q.get_covariance(), equal_nan=True) and p.SG == q.SG
    assert np.isnan(p.get_mlmc_variance()).all()
    p.estimate_missing_covariances(10)                                  # callable later, still nothing to do


LOADED = dict(np.load(os.path.join(GOLDEN, "pilot_loaded.npz")))
VARIANTS = sorted({k[:-len("_cov")] for k in LOADED if k.endswith("_cov")})


@pytest.mark.parametrize("variant", VARIANTS)
def test_paper_graph_files_load_as_in_the_reference(variant):
    PilotMixin, BLUEProblem = _classes()

    class P(PilotMixin, BLUEProblem):
        pass

    path = os.path.join(GOLDEN, "pilot_graph_%s.npz" % variant.split("_")[0])
    M = int(np.load(path)["M"])
    kw = {"costs": LOADED[variant + "_costs_in"]} if variant + "_costs_in" in LOADED else {}
    p = P(M, datafile=path, n_outputs=int(LOADED[variant + "_n_outputs"]), verbose=False, **kw)
    assert np.array_equal(np.array(p.get_covariances()), LOADED[variant + "_cov"], equal_nan=True)
    assert np.array_equal(np.array(p.get_mlmc_variances()), LOADED[variant + "_dV"], equal_nan=True)
    assert np.array_equal(p.get_costs(), LOADED[variant + "_costs"])
    assert np.array_equal(np.array(p.SG), LOADED[variant + "_SG"])
    assert len(VARIANTS) == 8


def _save_problem(**kw):
    PilotMixin, BLUEProblem = _classes()
    g = dict(np.load(os.path.join(GOLDEN, "pilot_save.npz")))

    class P(PilotMixin, BLUEProblem):
        pass

    return g, P, P(5, C=[c.copy() for c in g["in_C"]], costs=g["in_costs"], mlmc_variances=[d.copy() for d in g["in_dV"]],
                   n_outputs=2, verbose=False, **kw)


def test_save_writes_the_reference_arrays_and_round_trips(tmp_path):
    g, P, p = _save_problem()
    path = str(tmp_path / "graph.npz")
    p.save_graph_data(path)
    data = dict(np.load(path))
    assert sorted(data) == sorted(k[len("file_"):] for k in g if k.startswith("file_"))
    for k, v in data.items():
        ref = g["file_" + k]
        assert v.shape == ref.shape and v.dtype == ref.dtype, k
        assert np.array_equal(v, ref, equal_nan=True), k
    for n in range(2):                                                  # and the restated layout says the same
        assert np.array_equal(data["C%d" % n], pilot_ref.adjacency(g["in_C"][n]))
    q = P(5, datafile=path, n_outputs=2, verbose=False)
    assert np.array_equal(np.array(q.get_covariances()), np.array(p.get_covariances()), equal_nan=True)
    assert np.array_equal(np.array(q.get_mlmc_variances()), np.array(p.get_mlmc_variances()), equal_nan=True)
    assert np.array_equal(q.get_costs(), p.get_costs()) and q.SG == p.SG


def test_a_ragged_component_list_is_refused(tmp_path):
    from bluest_amd.sap import BLUESTError
    PilotMixin, BLUEProblem = _classes()

    class P(PilotMixin, BLUEProblem):
        pass

    C0 = np.array([[1.0, 0.5, 0.2], [0.5, 1.0, 0.3], [0.2, 0.3, 1.0]])
    C1 = C0.copy()
    C1[0, 2] = C1[2, 0] = C1[1, 2] = C1[2, 1] = np.inf                  # model 2 out of model 0's reach in output 1
    p = P(3, C=[C0, C1], costs=[3.0, 2.0, 1.0], n_outputs=2, verbose=False)
    assert [len(sg) for sg in p.SG] == [3, 2]
    with pytest.raises(BLUESTError, match="different sizes"):
        p.save_graph_data(str(tmp_path / "ragged.npz"))
    assert not os.path.exists(str(tmp_path / "ragged.npz"))


def test_a_file_of_another_problem_is_refused():
    PilotMixin, BLUEProblem = _classes()

    class P(PilotMixin, BLUEProblem):
        pass

    path = os.path.join(GOLDEN, "pilot_graph_matern.npz")              # M = 7, one output
    with pytest.raises(ValueError, match="mismatch"):
        P(6, datafile=path, verbose=False)
    with pytest.raises(ValueError, match="mismatch"):
        P(7, datafile=path, n_outputs=2, verbose=False)
    p = P(7, datafile=path, verbose=False)
    with pytest.raises(ValueError, match="mismatch"):
        p.load_graph_data(os.path.join(GOLDEN, "pilot_graph_hh.npz"))


def test_blueproblem_alone_still_refuses(tmp_path):
    from bluest_amd.sap import BLUESTError
    _, BLUEProblem = _classes()

    class B(BLUEProblem):
        def sampler(self, ls, N=1): pytest.fail("BLUEProblem alone never samples for an estimate")

    C = np.eye(3)
    with pytest.raises(BLUESTError):
        B(3, costs=[3.0, 2.0, 1.0], verbose=False)
    with pytest.raises(BLUESTError):
        B(3, C=C, verbose=False)
    with pytest.raises(BLUESTError):
        B(3, C=np.where(np.eye(3) > 0, 1.0, np.nan), costs=[3.0, 2.0, 1.0], verbose=False)
    with pytest.raises(BLUESTError):
        B(7, datafile=os.path.join(GOLDEN, "pilot_graph_matern.npz"), verbose=False)
    p = B(3, C=C, costs=[3.0, 2.0, 1.0], verbose=False)
    for call in (lambda: p.save_graph_data(str(tmp_path / "x.npz")), lambda: p.load_graph_data("x.npz"),
                 lambda: p.estimate_missing_covariances(10), lambda: p.estimate_costs()):
        with pytest.raises(BLUESTError):
            call()
    assert not hasattr(p, "blue_fn")


def test_sample_files_stay_refused():
    import bluest_amd
    from bluest_amd.sap import BLUESTError
    PilotMixin, BLUEProblem = _classes()

    class P(PilotMixin, BLUEProblem):
        def sampler(self, ls, N=1): return [np.zeros(N)] * len(ls)
        def evaluate(self, ls, samples, N=1): return [[s for s in samples]]

    with pytest.raises(BLUESTError):
        P(2, costs=[2.0, 1.0], samplefile="samples.npz", verbose=False)
    with pytest.raises(BLUESTError):
        bluest_amd.blue_fn([0], 2, P.__new__(P), outputs_to_save=[0], compute_mlmc_differences=True)
    p = P(2, C=np.eye(2), costs=[2.0, 1.0], verbose=False)
    for name in ("complexity_test", "variance_test", "reorder_graph_nodes", "reorder_all_graph_nodes"):
        with pytest.raises(BLUESTError):
            getattr(p, name)()

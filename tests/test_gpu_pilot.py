"""
GPU tests of bluest_amd.pilot.PilotMixin end to end: the reference fixtures (tools/gen_golden_pilot.py) replayed through the real
kernel, an exactly uncorrelated pair, the tutorial flow with nothing given but the costs, and MLMC on the estimated variances.
"""
import numpy as np
import pytest

import pilot_ref
from pilot_ref import cov_bound, scatter, within

pytestmark = pytest.mark.gpu

CASES = pilot_ref.case_names()


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.pilot import PilotMixin
    return PilotMixin, BLUEProblem


@pytest.mark.parametrize("name", CASES)
def test_fixture_through_the_kernel(name):
    """covariances and dV within 4 N u (sum|y_i y_j| / N + sum|y_i| sum|y_j| / N^2) per entry of the reference's (two summations
    of <= N terms each, in different orders; the analogous bound for dV), given entries exactly; the projected case then within
    the tolerance tests/test_gpu_covproj.py uses for projected covariances"""
    g = pilot_ref.case(name)
    N = int(g["N"])
    P = pilot_ref.replay_class(g, *_classes())
    p = P(skip_projection=True)
    assert p.calls == g["call_list"]
    if name == "inner":                                                 # Python inner products: host sums
        assert np.allclose(np.array(p.get_covariances()), g["cov"], rtol=1e-12, atol=1e-13, equal_nan=True)
        assert np.allclose(np.array(p.get_mlmc_variances()), g["dV"], rtol=1e-12, atol=1e-13, equal_nan=True)
    else:
        bc, bd = cov_bound(pilot_ref.pilot_values(g), N)
        within(np.array(p.get_covariances()), g["cov"] if bool(g["skip_projection"]) else g["cov_skip"], scatter(g, bc))
        within(np.array(p.get_mlmc_variances()), g["dV"], scatter(g, bd))
    assert np.array_equal(p.get_costs(), g["costs"])
    assert [list(sg) for sg in p.SG] == pilot_ref.unpadded(g["SG"])
    if not bool(g["skip_projection"]):
        q = P()                                                         # the fixture's own arguments: estimate, then project
        cov, ref = np.array(q.get_covariances()), g["cov"]
        for n in range(ref.shape[0]):
            scale = np.abs(g["cov_skip"][n][np.isfinite(g["cov_skip"][n])]).max()
            assert np.array_equal(np.isnan(cov[n]), np.isnan(ref[n])) and np.array_equal(cov[n] == 0.0, ref[n] == 0.0)
            known = ~np.isnan(ref[n])
            assert np.abs(cov[n][known] - ref[n][known]).max() <= 1e-8 * scale, np.abs(cov[n][known] - ref[n][known]).max()
        assert [list(sg) for sg in q.SG] == pilot_ref.unpadded(g["SG"])


def test_an_exactly_uncorrelated_pair():
    PilotMixin, BLUEProblem = _classes()
    table = np.array([[1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]])

    class P(PilotMixin, BLUEProblem):
        drawn = 0

        def sampler(self, ls, N=1):
            self.drawn += 1
            return [self.drawn - 1] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[float(table[l, samples[i]]) for i, l in enumerate(ls)]]

    kw = dict(costs=[2.0, 1.0], covariance_estimation_samples=4, verbose=False)
    p = P(2, **kw)
    assert np.array_equal(p.get_covariance(), np.array([[1.0, np.nan], [np.nan, 1.0]]), equal_nan=True)     # the pair is uncoupled
    assert p.SG == [[0]] and p.get_mlmc_variance()[0, 1] == 2.0
    q = P(2, remove_uncorrelated=False, **kw)
    assert np.array_equal(q.get_covariance(), np.eye(2)) and q.SG == [[0, 1]]                                # kept, at exactly 0


def model(n, l, z, e):
    """output n of model l: mean 1.5 (+ 0.1 n), correlated through z, own noise e"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def _tutorial_class(*bases):

    class P(*bases):
        def __init__(self, *a, **k):
            self.rng = np.random.RandomState(5)
            super().__init__(*a, **k)

        def sampler(self, ls, N=1):
            d = self.rng.randn(N, 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            Ps = [[model(n, l, *samples[i]) for i, l in enumerate(ls)] for n in range(self.n_outputs)]
            return [[float(v[0]) if len(v) == 1 else v for v in row] for row in Ps]
    return P


def test_tutorial_flow_with_nothing_given_but_the_costs():
    P = _tutorial_class(*_classes())
    costs = 4.0 ** -np.arange(5)
    p = P(5, n_outputs=2, costs=costs, covariance_estimation_samples=32, sample_batch_size=8, verbose=False)
    C = np.array(p.get_covariances())
    assert np.isfinite(C).all() and all(np.linalg.eigvalsh(c).min() > 0 for c in C) and p.SG == [list(range(5))] * 2
    eps = [0.05 * np.sqrt(c[0, 0]) for c in C]
    data = p.setup_solver(K=3, eps=eps)
    assert sorted(data) == ["errors", "models", "samples", "total_cost"] and (data["samples"] > 0).all()
    assert all(e <= 1.0002 * t for e, t in zip(data["errors"], eps))
    mus, errs, tot = p.solve(K=3, eps=eps)
    assert np.isfinite(mus).all() and tot == data["total_cost"] and abs(mus[0] - 1.5) < 0.5


def test_mlmc_uses_the_estimated_variances(capsys):
    from bluest_amd import misc
    from bluest_amd.mlmc import MLMCMixin
    PilotMixin, BLUEProblem = _classes()
    P = _tutorial_class(PilotMixin, MLMCMixin, BLUEProblem)
    costs = 4.0 ** -np.arange(5)
    p = P(5, n_outputs=2, costs=costs, covariance_estimation_samples=32, sample_batch_size=8, verbose=False)
    dV = p.get_mlmc_variances()
    iu = np.triu_indices(5, 1)
    assert all(np.isfinite(d[iu]).all() and (d[iu] > 0).all() for d in dV)
    data = p.setup_mlmc(eps=[0.05 * np.sqrt(c[0, 0]) for c in p.get_covariances()])
    assert "not provided nor estimated" not in capsys.readouterr().out
    group, samples = [int(l) for l in data["models"]], np.asarray(data["samples"])
    assert group[0] == 0 and len(group) > 1
    for n in range(2):                                                  # the level variances are the estimated dV, not C_ii + C_jj - 2 C_ij
        v, _ = misc.mlmc_levels(p.get_covariance(n), dV[n], costs, group)
        assert all(v[i] == dV[n][group[i], group[i + 1]] for i in range(len(group) - 1))
        assert abs(np.sqrt(sum(v / samples)) / data["errors"][n] - 1) < 1e-12
    q = _tutorial_class(MLMCMixin, BLUEProblem)(5, C=p.get_covariances(), n_outputs=2, costs=costs, verbose=False)
    q.setup_mlmc(eps=0.1)
    assert "not provided nor estimated" in capsys.readouterr().out      # the warning the mix-in makes unnecessary

"""
GPU test of bluest_amd.pilot_errors.PilotErrorsMixin end to end through the real kernels: a four-model Gaussian toy whose pilot
grows until every estimated entry meets covariance_estimation_tol, the sums of the last round against the long-double
restatement (tests/pilot4_ref.py), and the solver on the result.
"""
import numpy as np
import pytest

import pilot4_ref
from pilot4_ref import LD

pytestmark = pytest.mark.gpu

MIX = np.array([[1.0, 0.0, 0.0], [0.9, 0.3, 0.0], [0.7, 0.2, 0.4], [0.5, 0.1, 0.6]])


def test_the_pilot_grows_until_the_tolerance_holds_and_the_solver_runs(monkeypatch):
    from bluest_amd import pilot_errors
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.pilot import PilotMixin
    from bluest_amd.pilot_errors import PilotErrorsMixin
    calls = []
    real = pilot_errors.pilot_fourth_moments

    def recorded(values, *a, **k):
        out = real(values, *a, **k)
        calls.append((values, out))
        return out
    monkeypatch.setattr(pilot_errors, "pilot_fourth_moments", recorded)

    class P(PilotErrorsMixin, PilotMixin, BLUEProblem):
        def __init__(self, *a, **k):
            self.rng = np.random.RandomState(5)
            super().__init__(*a, **k)

        def sampler(self, ls, N=1):
            return [self.rng.randn(N, 3)] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[1.5 + samples[i] @ MIX[l] for i, l in enumerate(ls)]]

    tol, M = 0.15, 4
    costs = 4.0 ** -np.arange(M)
    p = P(M, costs=costs, covariance_estimation_samples=32, covariance_estimation_tol=tol, sample_batch_size=16, skip_projection=True,
          verbose=False)
    report = p.pilot_report
    assert report["converged"] is True and report["ratio"] <= 1 and report["rounds"] == len(calls) >= 2
    values, (_, first, s11, s21, s22, tpow) = calls[-1]
    N = values.shape[1]
    assert report["samples"] == N and [v.shape[1] for v, _ in calls] == sorted({v.shape[1] for v, _ in calls})
    # the sums of the last round: within (N + 16) u sum|term| of the long-double ones
    for name, got, ref, bound in zip(("first", "s11", "s21", "s22", "tpow"), (first, s11, s21, s22, tpow), pilot4_ref.sums_ld(values),
                                     pilot4_ref.bounds(values)):
        err = np.abs(got.astype(LD) - ref).astype(np.float64)
        assert (err <= bound).all(), name
    # the errors are the host arithmetic on those sums, bit for bit, at every entry (everything was estimated) ...
    se_c, se_d = pilot_errors.pilot_standard_errors(N, first, s11, s21, s22, tpow)
    assert np.array_equal(p.get_covariance_error(), se_c[0]) and np.array_equal(p.get_mlmc_variance_error(), se_d[0], equal_nan=True)
    # ... and agree with two passes in long double.  The one-pass form subtracts moments about the first sample, which lies
    # within a few standard deviations of the mean: the cancellation costs two or three digits of the sums' (N + 16) u ~ 1e-13
    ref_c, ref_d = pilot4_ref.standard_errors(values)
    iu = np.triu_indices(M, 1)
    assert np.abs(se_c[0] / ref_c[0] - 1).max() <= 1e-10 and np.abs(se_d[0][iu] / ref_d[0][iu] - 1).max() <= 1e-10
    # the criterion holds entry by entry
    C = p.get_covariance()
    sd = np.sqrt(np.diag(C))
    assert (se_c[0] <= tol * np.outer(sd, sd) * (1 + 1e-9)).all()
    assert (se_d[0][iu] <= tol * p.get_mlmc_variance()[iu] * (1 + 1e-9)).all()
    # the estimates are PilotMixin's on the same samples, and the solver runs on them unchanged
    truth = MIX @ MIX.T
    assert (np.abs(C - truth) <= 5 * se_c[0]).all()
    eps = 0.05 * np.sqrt(C[0, 0])
    data = p.setup_solver(K=3, eps=eps)
    assert sorted(data) == ["errors", "models", "samples", "total_cost"] and data["errors"][0] <= 1.0002 * eps
    mus, errs, tot = p.solve(K=3, eps=eps)
    assert np.isfinite(mus).all() and tot == data["total_cost"] and abs(mus[0] - 1.5) < 0.5

"""
GPU tests of bluest_amd.field_covariances.FieldCovariancesMixin end to end through the real kernels and the real allocation: the
seeded problem of tests/test_gpu_field_errors.py, four models with one number (d = 1) and one field of d = 5 components per model,
whose covariance in the inner product is known.  solve() keeps the bits of FieldOutputsMixin.solve(); the error bar is
FieldErrorsMixin's on the same draws, and for a number the group covariances are MomentsMixin's, both to a rounding bound; the
pooled covariance lies within 5 Wishart standard errors of the true one; and a problem set up with the pooled covariance solves.

The rounding bound.  u' C^ u and the sampled variance of z = u' y are the same quantity, but the BLUE weights cancel (u has both
signs), so the bound is relative to the magnitudes, not to the result: gamma sum_jk |u_j| |u_k| sqrt(C^_jj C^_kk) with
gamma = 4 (N + d + L) 2^-52 -- N + d additions and fmas per entry of `second`, L per chain of z, and the factor 4 for the two
sums (second and cross, zsq and zsum) and the two roundings of each product.
"""
import numpy as np
import pytest

from gsums_ref import same_bits
from test_gpu_field_errors import M, exact_covariance, problem, segments_drawn, shape_of

pytestmark = pytest.mark.gpu

D = 5


def _bases(errors=False):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_covariances import FieldCovariancesMixin
    from bluest_amd.field_errors import FieldErrorsMixin
    from bluest_amd.fields import FieldOutputsMixin
    return (FieldCovariancesMixin,) + ((FieldErrorsMixin,) if errors else ()) + (FieldOutputsMixin, SamplingMixin, BLUEProblem)


def gamma(N, d, L):
    return 4 * (N + d + L) * 2.0 ** -52


@pytest.fixture(scope="module")
def solved():
    """the problem with both mix-ins, solved once, and the parent's solve on the same seed"""
    bases = _bases(errors=True)
    plain = problem(bases[2:], D)
    want = plain.solve(K=3, eps=plain.test_eps)
    p = problem(bases, D)
    got = p.solve(K=3, eps=p.test_eps)
    return plain, want, p, got


def test_solve_keeps_its_bits_and_the_covariances_are_those_of_the_draw(solved):
    plain, want, p, (mus, errs, cost) = solved
    assert p.calls == plain.calls and np.array_equal(p.MOSAP_output["samples"], plain.MOSAP_output["samples"])
    assert same_bits(mus[0], want[0][0]) and same_bits(mus[1], want[0][1]) and same_bits(errs, want[1]) and cost == want[2]
    assert isinstance(mus[0], float) and mus[1].shape == (D,)
    samples = np.asarray(p.MOSAP_output["samples"])
    chosen = np.flatnonzero(samples > 0).tolist()
    weights = [np.ones(1), shape_of(D)[1]]
    assert sorted(p.field_sample_covariances[0]) == sorted(p.field_sample_covariances[1]) == chosen
    for g, vals in segments_drawn(p):
        for n in range(2):
            N, C = p.field_sample_covariances[n][g]
            y = vals[n]
            assert N == int(samples[g]) == y.shape[0] and C.shape == (y.shape[1],) * 2
            if N >= 2:
                dm = y - y.mean(axis=0, keepdims=True)
                assert np.allclose(C, np.einsum("ijc,c,ikc->jk", dm, weights[n], dm) / (N - 1), rtol=1e-10, atol=0), (n, g)
            else:
                assert np.isnan(C).all()
    assert np.allclose(p.sampled_errors(source="model"), errs, rtol=1e-15, atol=0)  # solve()'s errors back


def test_the_error_bar_is_the_one_of_the_field_errors_on_the_same_draws(solved):
    from bluest_amd.field_errors import FieldErrorsMixin
    _, _, p, _ = solved
    a, b = p.sampled_errors(), FieldErrorsMixin.sampled_errors(p)
    samples = np.asarray(p.MOSAP_output["samples"])
    W = p._blue_weights()[0]
    bound, c = np.zeros(2), 0
    for g in np.flatnonzero(samples > 0).tolist():
        L = len(p.MOSAP_output["flattened_groups"][g])
        for n, d in enumerate((1, D)):
            N, C = p.field_sample_covariances[n][g]
            if N >= 2:
                s = np.abs(W[n, c:c + L]) * np.sqrt(np.diag(C))
                bound[n] += samples[g] * gamma(N, d, L) * s.sum() ** 2
        c += L
    print("variances from the covariances", a ** 2, "from the field errors", b ** 2, "difference", np.abs(a ** 2 - b ** 2), "bound", bound)
    assert (np.abs(a ** 2 - b ** 2) <= bound).all()
    assert np.allclose(a, b, rtol=1e-9, atol=0)


def test_for_a_number_the_group_covariances_are_those_of_the_moments():
    """the same problem with its number alone, on the same draws: a field of one component here, MomentsMixin there"""
    from bluest_amd.moments import MomentsMixin
    bases = _bases()
    p = problem(bases, 1, with_field=False)
    r = problem((MomentsMixin,) + bases[2:], 1, with_field=False)
    (mus, errs, cost), (mus_r, errs_r, cost_r) = p.solve(K=3, eps=p.test_eps), r.solve(K=3, eps=r.test_eps)
    assert p.calls == r.calls and np.array_equal(p.MOSAP_output["samples"], r.MOSAP_output["samples"])
    assert same_bits(mus, mus_r) and same_bits(errs, errs_r) and cost == cost_r
    for g, (N, C) in p.field_sample_covariances[0].items():
        N_r, C_r = r.sample_moments[g]
        assert N == N_r
        if N >= 2:
            scale = np.sqrt(np.outer(np.diag(C), np.diag(C)))
            assert (np.abs(C - C_r[0]) <= gamma(N, 1, C.shape[0]) * scale).all(), g
        else:
            assert np.isnan(C).all() and np.isnan(C_r[0]).all()
    Cs, dof = p.pooled_covariances()
    Cs_r, dof_r = r.pooled_covariances()
    assert np.array_equal(dof[0], dof_r[0]) and np.allclose(Cs[0], Cs_r[0], rtol=1e-12, atol=0)
    assert np.allclose(p.sampled_errors(), r.sampled_errors(), rtol=1e-12, atol=0)


def test_the_pooled_covariance_is_the_true_one_to_sampling_and_solves_again(solved):
    """every pooled entry within 5 Wishart standard errors sqrt((C_ii C_jj + C_ij^2) / dof) of the true covariance in the inner
    product; then the pooled matrices go on as C of a new problem, which solves and promises finite errors"""
    _, _, p, _ = solved
    amp, mass = shape_of(D)
    true = [exact_covariance(0), float(np.dot(amp * mass, amp)) * exact_covariance(1)]
    Cs, dofs = p.pooled_covariances()
    for n in range(2):
        C, dof = true[n], dofs[n]
        assert np.allclose(Cs[n], Cs[n].T, rtol=1e-13) and (dof > 0).any()     # (a model no group was drawn twice with keeps its entries)
        se = np.sqrt((np.outer(np.diag(C), np.diag(C)) + C * C) / np.maximum(dof, 1))
        ratio = np.abs(Cs[n] - C) / se
        print("output", n, "dof", dof.tolist(), "largest |pooled - true| / standard error", ratio.max())
        assert (ratio[dof > 0] <= 5).all() and same_bits(Cs[n][dof == 0], C[dof == 0])
    bases = _bases()
    q = problem(bases[1:], D, seed=8)
    again = type(q)(M, C=Cs, costs=2.0 ** -np.arange(M), n_outputs=2, verbose=False, sample_batch_size=32)
    again.rng, again.drawn, again.calls = np.random.RandomState(8), [], []
    mus, errs, cost = again.solve(K=3, eps=q.test_eps)
    assert np.isfinite(errs).all() and (np.asarray(errs) > 0).all() and np.isfinite(mus[1]).all() and np.isfinite(cost)

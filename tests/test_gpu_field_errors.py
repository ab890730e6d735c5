"""
GPU tests of bluest_amd.field_errors.FieldErrorsMixin end to end through the real kernels and the real allocation: a seeded problem of
four models with one number and one field of d = 1, 5 or 70 components per model (the toy model of tests/test_gpu_fields.py).
solve() keeps the bits of FieldOutputsMixin.solve(); field_sample_moments is the variance of the weighted combination of the very
samples that were drawn; the error in the norm and the map are the stated formulas, evaluated by numpy on the same draws;
source="model" gives solve()'s errors back; values that stay on the device give the same bits; and for an output that is a number
the error bar is MomentsMixin's.
"""
import numpy as np
import pytest

from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

M = 4


def model(n, l, z, e):
    """the toy model of tests/test_gpu_estimator.py"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def exact_covariance(n):
    a, d = 1 + 0.3 * n, 0.1 * n
    b, c = 0.9 ** np.arange(M), 0.1 * (np.arange(M) + 1)
    return a * a * np.outer(b, b) + 2 * d * d + np.diag(a * a * c * c)


def shape_of(d):
    """the field's amplitudes per component and the weights of its inner product"""
    c = np.arange(d)
    return 0.5 + 0.3 * (c % 7) - 1.0 * (c % 3 == 1), (1.0 + (c % 3)) / d


def problem(bases, d, seed=7, on_device=False, with_field=True):
    """one number and (with_field) one field of d components per model, drawn in batches of 32; evaluate records what it returns"""
    amp, mass = shape_of(d)

    class Toy(*bases):
        def sampler(self, ls, N=1):
            self.calls.append((list(ls), int(N)))
            z = self.rng.randn(int(N), 1 + len(ls))
            return [(z[:, 0], z[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            Ps = [[model(0, l, *samples[i]) for i, l in enumerate(ls)]]
            if with_field:
                Ps.append([amp[None, :] * model(1, l, *samples[i])[:, None] + np.arange(d)[None, :] for i, l in enumerate(ls)])
            self.drawn.append((list(ls), Ps))
            if on_device:
                import torch
                return [[torch.from_numpy(np.ascontiguousarray(v)).cuda() for v in row] for row in Ps]
            return Ps

    if any(b.__name__ == "FieldOutputsMixin" for b in bases):
        Toy.output_weights = lambda self: [None, mass] if with_field else [None]
    cov = [exact_covariance(0)] + ([float(np.dot(amp * mass, amp)) * exact_covariance(1)] if with_field else [])
    p = Toy(M, C=cov, costs=2.0 ** -np.arange(M), n_outputs=len(cov), verbose=False, sample_batch_size=32)
    p.rng, p.drawn, p.calls = np.random.RandomState(seed), [], []
    p.test_eps = [0.1] + ([0.1 * float(np.sqrt(cov[1][0, 0]))] if with_field else [])
    return p


def _bases():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_errors import FieldErrorsMixin
    from bluest_amd.fields import FieldOutputsMixin
    return FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem


def segments_drawn(p):
    """per sampled group (in list order) and output the values [N, L, d_n] that p drew"""
    out = p.MOSAP_output
    samples = np.asarray(out["samples"])
    segs, k = [], 0
    for g in np.flatnonzero(samples > 0).tolist():
        need, parts = int(samples[g]), [[] for _ in range(p.n_outputs)]
        while need > 0:
            ls, Ps = p.drawn[k]
            assert ls == [int(l) for l in out["flattened_groups"][g]]
            for n in range(p.n_outputs):
                block = np.stack([np.asarray(v) for v in Ps[n]], axis=1)
                parts[n].append(block[:, :, None] if block.ndim == 2 else block)
            need -= parts[0][-1].shape[0]
            k += 1
        assert need == 0
        segs.append((g, [np.concatenate(x) for x in parts]))
    assert k == len(p.drawn)
    return segs


@pytest.mark.parametrize("d", [1, 5, 70])
def test_solve_keeps_its_bits_and_the_error_bars_are_those_of_the_draw(d):
    bases = _bases()
    amp, mass = shape_of(d)
    plain = problem(bases[1:], d)
    want = plain.solve(K=3, eps=plain.test_eps)
    p = problem(bases, d)
    mus, errs, cost = p.solve(K=3, eps=p.test_eps)
    assert p.calls == plain.calls and np.array_equal(p.MOSAP_output["samples"], plain.MOSAP_output["samples"])
    assert same_bits(mus[0], want[0][0]) and same_bits(mus[1], want[0][1]) and same_bits(errs, want[1]) and cost == want[2]
    assert isinstance(mus[0], float) and mus[1].shape == (d,)

    samples = np.asarray(p.MOSAP_output["samples"])
    chosen = np.flatnonzero(samples > 0).tolist()
    segs = segments_drawn(p)
    W = p._blue_weights()[0]
    weights = [np.ones(1), mass]
    norm, maps, unsampled, c = np.zeros(2), [np.zeros(1), np.zeros(d)], [0.0, 0.0], 0
    for g, vals in segs:
        ls, m = [int(l) for l in p.MOSAP_output["flattened_groups"][g]], int(samples[g])
        for n in range(2):
            N, var = p.field_sample_moments[n][g]
            assert N == m == vals[n].shape[0] and var.shape == ((1, d)[n],)
            w = W[n, c:c + len(ls)]
            if m >= 2:
                z = np.einsum("j,ijc->ic", w, vals[n])
                assert np.allclose(var, z.var(axis=0, ddof=1), rtol=1e-10, atol=0), (n, g)
                norm[n] += m * float(np.dot(weights[n], z.var(axis=0, ddof=1)))
                maps[n] += m * z.var(axis=0, ddof=1)
            else:
                assert np.isnan(var).all()
                if w.any():
                    share = m * float(w @ p.get_covariance(n)[np.ix_(ls, ls)] @ w)
                    norm[n] += share
                    unsampled[n] += share
        c += len(ls)
    assert sorted(p.field_sample_moments[0]) == sorted(p.field_sample_moments[1]) == chosen
    sampled = p.sampled_errors()
    print("d", d, "samples", samples[chosen], "sampled_errors()", sampled, "promised", errs)
    assert np.allclose(sampled, np.sqrt(norm), rtol=1e-10, atol=0)
    assert (sampled > 0.5 * errs).all() and (sampled < 2.0 * errs).all()            # the model is the truth here, up to sampling
    assert np.allclose(p.sampled_errors(source="model"), errs, rtol=1e-15, atol=0)  # solve()'s errors back
    got_maps, got_unsampled = p.sampled_error_fields()
    assert isinstance(got_maps[0], float) and got_maps[1].shape == (d,)
    assert np.allclose(got_maps[0], np.sqrt(maps[0][0]), rtol=1e-10) and np.allclose(got_maps[1], np.sqrt(maps[1]), rtol=1e-10, atol=0)
    assert np.allclose(got_unsampled, unsampled, rtol=1e-10, atol=0)
    # component c of the field is amp[c] times one random number (plus a constant): the map is |amp| times one standard error
    ratio = got_maps[1] / np.abs(amp)
    assert np.allclose(ratio, ratio[0], rtol=1e-9)

    # device-resident values: evaluate returns CUDA tensors, the same bits come out
    q = problem(bases, d, on_device=True)
    mus_dev, errs_dev, _ = q.solve(K=3, eps=q.test_eps)
    assert q.calls == p.calls and same_bits(mus_dev[0], mus[0]) and same_bits(mus_dev[1], mus[1]) and same_bits(errs_dev, errs)
    for n in range(2):
        for g in chosen:
            assert q.field_sample_moments[n][g][0] == p.field_sample_moments[n][g][0]
            assert np.array_equal(q.field_sample_moments[n][g][1], p.field_sample_moments[n][g][1], equal_nan=True)
    assert same_bits(q.sampled_errors(), sampled)


def test_for_a_number_the_error_bar_is_the_one_of_the_group_covariances():
    """the same problem with its number alone, on the same draws: sum_g m_g Var(u' y) here, sum_g m_g u' C^ u in MomentsMixin"""
    from bluest_amd.moments import MomentsMixin
    bases = _bases()
    p = problem(bases, 1, with_field=False)
    r = problem((MomentsMixin,) + bases[2:], 1, with_field=False)
    (mus, errs, cost), (mus_r, errs_r, cost_r) = p.solve(K=3, eps=p.test_eps), r.solve(K=3, eps=r.test_eps)
    assert p.calls == r.calls and np.array_equal(p.MOSAP_output["samples"], r.MOSAP_output["samples"])
    assert same_bits(mus, mus_r) and same_bits(errs, errs_r) and cost == cost_r
    a, b = p.sampled_errors(), r.sampled_errors()
    print("field errors", a, "group covariances", b, "relative difference", np.abs(a / b - 1))
    assert np.allclose(a, b, rtol=1e-12, atol=0)
    assert np.allclose(p.sampled_errors(source="model"), errs, rtol=1e-15, atol=0)
    maps, unsampled = p.sampled_error_fields()
    assert isinstance(maps[0], float) and np.isclose(maps[0] ** 2 + unsampled[0], a[0] ** 2, rtol=1e-12)

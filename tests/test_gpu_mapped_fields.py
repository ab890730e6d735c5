"""GPU tests of bluest_amd.field_maps.MappedFieldsMixin end to end.  Three models of a smooth random field on 1-D grids of 17, 9
and 5 nodes, mapped by linear interpolation onto the 17 nodes of model 0 (whose operator is None) with trapezoid weights, and a
second output that is a number; every covariance comes from 40 pilot samples.  The TWIN is the same class without the mix-in
whose evaluate maps on the host side of the interface -- with the numpy restatement (tests/field_map_ref.py) once, with
map_fields otherwise: the mix-in must give the twin's bits everywhere, with the twin's sampler calls, a batch with a non-finite
raw value included, alone and under each of the three mix-ins that stack on FieldOutputsMixin.  And one check of meaning: with
every model a restriction of the SAME fine field, dV is the weighted norm of (B P - I) y."""
import numpy as np
import pytest

import field_map_ref as ref
from field_map_ref import same_bits

pytestmark = pytest.mark.gpu

NODES = [17, 9, 5]
M, Q = 3, 17
X = [np.linspace(0.0, 1.0, n) for n in NODES]
W = np.full(Q, 1.0 / (Q - 1))
W[[0, -1]] *= 0.5                                                       # trapezoid weights on the common grid
CSR = [None, ref.interpolation_1d(9, 17), ref.interpolation_1d(5, 17)]
COSTS = [1.0, 0.25, 0.0625]
BUDGET = 40.0


def raw_field(l, z, e):
    """[N2, NODES[l]]: model l of the field on its own grid; z is shared by the models of a sample, e is the model's own"""
    x = X[l][None, :]
    return ((1.0 + 0.5 * z)[:, None] * np.sin(np.pi * x) + 0.3 * (z ** 2)[:, None] * x + (0.1 * (l + 1) * e)[:, None] * np.cos(np.pi * x) * x)


def number(l, z, e):
    return 1.5 + 0.9 ** l * z + 0.1 * (l + 1) * e


def problem(kind, extra=(), on_device=False, poison=None, seed=5, **kw):
    """kind "mapped": the mix-in, evaluate returns each model's own nodes; "twin_ref" / "twin_gpu": no mix-in, evaluate returns
    the mapped fields, mapped by the restatement / by map_fields.  `poison`: the sampler call whose batch holds one infinite RAW
    value (once).  The sampler records its calls; _field_segments_flushed records what reaches it."""
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_maps import FieldOperator, MappedFieldsMixin, map_fields
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.pilot import PilotMixin
    ops = [None if c is None else FieldOperator(c[:3], shape=c[3]) for c in CSR]

    class Toy(*(((MappedFieldsMixin,) if kind == "mapped" else ()) + tuple(extra) + (FieldOutputsMixin, SamplingMixin, PilotMixin, BLUEProblem))):
        rng, calls, flushed, poisoned = np.random.RandomState(seed), [], [], []

        def output_weights(self): return [W, None]

        def sampler(self, ls, N=1):
            self.calls.append((list(ls), int(N)))
            d = self.rng.randn(int(N), 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            fields = [raw_field(l, *samples[i]) for i, l in enumerate(ls)]
            if poison == len(self.calls) and not self.poisoned:
                self.poisoned.append(True)
                fields[-1][0, 2] = np.inf
            if kind != "mapped":
                if kind == "twin_ref":
                    both = ref.map_fields(fields, [CSR[l] for l in ls])
                else:
                    both = map_fields(fields, [ops[l] for l in ls])
                fields = [np.ascontiguousarray(both[:, i]) for i in range(len(ls))]
            numbers = [number(l, *samples[i]) for i, l in enumerate(ls)]
            if on_device:
                import torch
                return [[torch.from_numpy(v).cuda() for v in row] for row in (fields, numbers)]
            return [fields, numbers]

        def _field_segments_flushed(self, where, n, segments):
            self.flushed.append((n, segments))
            return super()._field_segments_flushed(where, n, segments)

    if kind == "mapped":
        Toy.output_operators = lambda self: [ops, None]
    return Toy(M, costs=np.array(COSTS), n_outputs=2, verbose=False, sample_batch_size=16, skip_projection=True,
               covariance_estimation_samples=40, **kw)


def same(a, b):
    """bit for bit through lists, tuples and dicts"""
    if isinstance(a, dict):
        return isinstance(b, dict) and sorted(a) == sorted(b) and all(same(a[k], b[k]) for k in a)
    if isinstance(a, (list, tuple)):
        return isinstance(b, (list, tuple)) and len(a) == len(b) and all(same(x, y) for x, y in zip(a, b))
    if a is None or b is None or isinstance(a, (str, bool)):
        return a is b or a == b
    return same_bits(np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64))


def same_pilot(p, t):
    iu = np.triu_indices(M, 1)
    return (same_bits(np.array(p.get_covariances()), np.array(t.get_covariances())) and np.array_equal(p.get_costs(), t.get_costs())
            and same_bits(np.array(p.get_mlmc_variances())[:, iu[0], iu[1]], np.array(t.get_mlmc_variances())[:, iu[0], iu[1]]))


def test_pilot_allocation_and_solve_are_those_of_the_host_mapped_twin():
    p, t = problem("mapped"), problem("twin_ref")
    assert p.calls == t.calls == [([0, 1, 2], 16), ([0, 1, 2], 16), ([0, 1, 2], 8)]
    assert same_pilot(p, t) and np.all(np.isfinite(p.get_covariance(0))) and np.all(np.diag(p.get_covariance(0)) > 0)
    got, want = p.solve(K=3, budget=BUDGET), t.solve(K=3, budget=BUDGET)
    assert np.array_equal(p.MOSAP_output["samples"], t.MOSAP_output["samples"]) and p.MOSAP_output["samples"].sum() > 0
    assert p.calls == t.calls and len(p.calls) > 3
    assert np.asarray(got[0][0]).shape == (Q,) and isinstance(got[0][1], float)      # the estimate lives in the common space
    assert same(got, want)
    field_segments = [s for n, segs in p.flushed if n == 0 for s in segs]
    assert field_segments and all(isinstance(s, np.ndarray) and s.shape[2] == Q for s in field_segments)


def test_variance_test_and_a_redrawn_batch_are_those_of_the_twin():
    p, t = problem("mapped", poison=2), problem("twin_gpu", poison=2)
    assert p.calls == t.calls == [([0, 1, 2], 16), ([0, 1, 2], 16), ([0, 1, 2], 16), ([0, 1, 2], 8)]       # the second batch, asked again
    assert p.poisoned and t.poisoned and same_pilot(p, t)
    assert same(p.variance_test(budget=BUDGET, K=3, N=5), t.variance_test(budget=BUDGET, K=3, N=5))
    assert np.array_equal(p.MOSAP_output["samples"], t.MOSAP_output["samples"]) and p.calls == t.calls
    q, u = problem("mapped", poison=5), problem("twin_gpu", poison=5)  # and in the main run: the first batch of the estimator
    assert same(q.solve(K=3, budget=BUDGET), u.solve(K=3, budget=BUDGET))
    assert q.poisoned and q.calls == u.calls and q.calls[5] == q.calls[4]


def test_cuda_batches_stay_on_the_device_and_give_the_same_bits():
    import torch
    p, h = problem("mapped", on_device=True), problem("mapped")
    assert same_pilot(p, h) and same(p.solve(K=3, budget=BUDGET), h.solve(K=3, budget=BUDGET)) and p.calls == h.calls
    field_segments = [s for n, segs in p.flushed if n == 0 for s in segs]
    assert field_segments and all(isinstance(s, torch.Tensor) and s.is_cuda and s.shape[2] == Q for s in field_segments)
    assert all(same_bits(a.cpu().numpy(), b) for a, b in zip(field_segments, [s for n, segs in h.flushed if n == 0 for s in segs]))


def test_under_field_errors_the_error_maps_are_those_of_the_twin():
    from bluest_amd.field_errors import FieldErrorsMixin
    p, t = problem("mapped", extra=(FieldErrorsMixin,)), problem("twin_gpu", extra=(FieldErrorsMixin,))
    assert same(p.solve(K=3, budget=BUDGET), t.solve(K=3, budget=BUDGET))
    maps, unsampled = p.sampled_error_fields()
    assert np.asarray(maps[0]).shape == (Q,) and same((maps, unsampled), t.sampled_error_fields())
    assert same(p.sampled_errors(), t.sampled_errors())


def test_under_field_covariances_the_pooled_covariances_are_those_of_the_twin():
    from bluest_amd.field_covariances import FieldCovariancesMixin
    p, t = problem("mapped", extra=(FieldCovariancesMixin,)), problem("twin_gpu", extra=(FieldCovariancesMixin,))
    assert same(p.solve(K=3, budget=BUDGET), t.solve(K=3, budget=BUDGET))
    assert same(p.pooled_covariances(), t.pooled_covariances()) and same(p.sampled_errors(), t.sampled_errors())


def test_under_field_pilot_errors_the_adaptive_pilot_is_that_of_the_twin():
    from bluest_amd.field_pilot_errors import FieldPilotErrorsMixin
    p, t = (problem(kind, extra=(FieldPilotErrorsMixin,), covariance_estimation_tol=0.2) for kind in ("mapped", "twin_gpu"))
    print(p.pilot_report)
    assert p.pilot_report == t.pilot_report and p.pilot_report["rounds"] >= 2 and p.calls == t.calls      # mapped rounds are joined
    assert same_pilot(p, t) and same(p.get_covariance_errors(), t.get_covariance_errors())
    assert same(p.get_mlmc_variance_errors(), t.get_mlmc_variance_errors())


def test_dv_is_the_weighted_norm_of_the_interpolation_error():
    """every model is the restriction (injection P_l: every 2^l-th node) of the SAME fine field y, so model 0 minus mapped model l
    is (I - B_l P_l) y, and dV[0, l] = mean <D, D>_w - <mean D, mean D>_w over the pilot samples (bluest_amd/pilot.py)"""
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.field_maps import MappedFieldsMixin
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.pilot import PilotMixin

    class Nested(MappedFieldsMixin, FieldOutputsMixin, PilotMixin, BLUEProblem):
        rng, fine = np.random.RandomState(3), []

        def output_weights(self): return [W]

        def output_operators(self): return [[None if c is None else (c[:3], c[3]) for c in CSR]]

        def sampler(self, ls, N=1):
            z = self.rng.randn(int(N), 3)
            return [z] * len(ls)

        def evaluate(self, ls, samples, N=1):
            z, x = samples[0], X[0][None, :]
            y = z[:, :1] * np.sin(np.pi * x) + z[:, 1:2] * np.sin(3 * np.pi * x) + z[:, 2:] * x ** 2
            self.fine.append(y)
            return [[np.ascontiguousarray(y[:, ::2 ** l]) for l in ls]]

    p = Nested(M, costs=np.array(COSTS), n_outputs=1, verbose=False, sample_batch_size=16, skip_projection=True, covariance_estimation_samples=40)
    Y = np.concatenate(p.fine)
    assert Y.shape == (40, Q)
    dV = p.get_mlmc_variance(0)
    for l in (1, 2):
        B = np.asarray(ref.dense(CSR[l]), dtype=np.float64)
        D = Y - Y[:, ::2 ** l] @ B.T
        want = np.mean((D * D) @ W) - float(np.dot(D.mean(axis=0) ** 2, W))
        print("model", l, "dV", dV[0, l], "numpy", want)
        assert want > 0 and abs(dV[0, l] - want) <= 1e-12 * want

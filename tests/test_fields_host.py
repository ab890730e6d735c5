"""CPU tests of bluest_amd.fields: the restated summation order of Part 12 against the reference's recorded sums for a weighted
inner product (tests/golden/pilot_case_inner.npz), the FieldOutputsMixin flow over those pilot samples with the GPU call replaced
by the long-double stand-in of tests/fields_ref.py, the derived inner products, and the refusals."""
import numpy as np
import pytest

import fields_ref
import pilot_ref
from pilot_ref import scatter, within


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.pilot import PilotMixin
    return FieldOutputsMixin, PilotMixin, BLUEProblem


def inner_values():
    """the fixture's pilot samples per output, [N, L, d], and its weights"""
    g = pilot_ref.case("inner")
    Y = np.stack(g["blocks"], axis=1)                                   # [n_out, N, L, d]
    return g, [np.ascontiguousarray(Y[n]) for n in range(Y.shape[0])], g["vec_weights"]


def test_both_entry_points_are_bound():
    from bluest_amd import _lib
    assert len(_lib.SIGNATURES["bluest_field_stats"]) == 10 and len(_lib.SIGNATURES["bluest_field_sums"]) == 11
    L = _lib.lib()
    assert hasattr(L, "bluest_field_stats") and hasattr(L, "bluest_field_sums") and L.bluest_abi_version() == 1


def test_restated_order_reproduces_the_reference_sums():
    """|restatement - reference| <= 4 n u sum|terms|, n = N d: both are sums of at most n rounded terms in different orders"""
    g, values, w = inner_values()
    for n, Y in enumerate(values):
        assert Y.shape == (int(g["N"]), len(g["ls"]), len(w))
        se, sc, flat, d2 = fields_ref.field_stats(Y, w)
        iu = fields_ref.pairs(Y.shape[1])
        d1 = np.zeros(Y.shape[1:2] * 2 + Y.shape[2:])
        d1[iu[0], iu[1]] = flat
        bounds = fields_ref.sum_bounds(Y, w)
        for name, mine, ref, bound in zip(("sumse", "sumsc", "sumsd1", "sumsd2"), (se, sc, d1, d2),
                                          (g["fn_sumse"][n], g["fn_sumsc"][n], g["fn_sumsd1"][n], g["fn_sumsd2"][n]), bounds):
            err = np.abs(mine - ref)
            print(name, "largest error / bound:", float((err[bound > 0] / bound[bound > 0]).max()))
            assert (err <= bound).all(), name
        assert fields_ref.same_bits(sc, sc.T) and not np.tril(d2).any()
        # and the long-double sums agree with the restatement to the same bound
        for mine, ld, bound in zip((se, sc, d1, d2), fields_ref.stats_ld(Y, w)[0], bounds):
            assert (np.abs(mine - np.asarray(ld, dtype=np.float64)) <= bound).all()


def test_restated_group_sums_are_part_11_per_component():
    import gsums_ref
    rng = np.random.RandomState(3)
    v = rng.randn(300, 3, 5)
    got = fields_ref.segment_sums(v)
    for c in range(5):
        assert fields_ref.same_bits(got[:, c], gsums_ref.segment_sums(np.ascontiguousarray(v[None, :, :, c]))[0])
    ld, mag = fields_ref.segment_ld(v)
    assert (np.abs(got - np.asarray(ld, dtype=np.float64)) <= 300 * fields_ref.U * np.asarray(mag, dtype=np.float64)).all()
    sums, mu = fields_ref.field_group_sums([v, v[:7, :2]], weights=[0.5, -1.0, 2.0, 3.0, 0.25], repeat_of=[0, 2])
    assert mu.shape == (3, 5) and not mu[1].any()
    assert np.allclose(mu[0], 0.5 * sums[0][0] - sums[0][1] + 2 * sums[0][2], rtol=1e-14)
    assert np.allclose(mu[2], 3 * sums[1][0] + 0.25 * sums[1][1], rtol=1e-14)


def test_mixin_reproduces_the_reference_with_one_call_per_output(monkeypatch):
    from bluest_amd import fields
    g, values, w = inner_values()
    calls = []

    def stats(vals, weights, differences=True):
        calls.append((vals.shape, np.array(weights)))
        return fields_ref.field_statistics(vals, weights, differences)
    monkeypatch.setattr(fields, "field_statistics", stats)

    class P(pilot_ref.replay_class(g, *_classes())):
        def output_weights(self): return [w.copy() for n in range(self.n_outputs)]

    p = P(skip_projection=True)
    assert p.calls == g["call_list"]                                   # the reference's sampler calls, in its order
    N, L, d = int(g["N"]), len(g["ls"]), len(w)
    assert [c[0] for c in calls] == [(N, L, d)] * int(g["n_outputs"])  # ONE statistics call per output with all the values
    assert all(np.array_equal(c[1], w) for c in calls)
    bounds = [fields_ref.cov_bound(Y, w, N) for Y in values]
    within(np.array(p.get_covariances()), g["cov"], scatter(g, np.stack([b[0] for b in bounds])))
    within(np.array(p.get_mlmc_variances()), g["dV"], scatter(g, np.stack([b[1] for b in bounds])))
    assert np.array_equal(p.get_costs(), g["costs"])
    assert [list(sg) for sg in p.SG] == pilot_ref.unpadded(g["SG"])


def _toy(*bases, weights, **kw):
    class Toy(*bases):
        def output_weights(self): return weights
        def sampler(self, ls, N=1): return [np.zeros(N)] * len(ls)
    C = np.array([[1.0, 0.5], [0.5, 1.0]])
    return Toy(2, C=[C] * len(weights), costs=[2.0, 1.0], n_outputs=len(weights), verbose=False, **kw)


def test_inner_products_are_derived_from_the_declared_weights():
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.sap import BLUESTError
    F, PM, B = _classes()
    w = np.array([1.0, 0.5, 2.0])
    p = _toy(F, SamplingMixin, B, weights=[None, w])
    scalar, field = p.get_models_inner_products()
    assert scalar(3.0, -2.0) == -6.0
    a, b = np.array([1.0, 2.0, 3.0]), np.array([-1.0, 4.0, 0.5])
    assert field(a, b) == float(np.dot(a * w, b)) and isinstance(field(a, b), float)
    assert p._host_outputs() is False
    q = _toy(F, PM, B, weights=[None, w])
    assert q.outer([a, b], [a, b], q.get_models_inner_products()[1])[0, 1] == field(a, b)       # PilotMixin's host formula
    p.output_weights = lambda: [None]                                   # one entry per output
    with pytest.raises(BLUESTError):
        p.get_models_inner_products()
    del p.output_weights
    for bad in ([None, np.array([1.0, -1.0])], [None, np.array([np.nan])], [None, np.ones((2, 2))], [None, np.ones(0)]):
        with pytest.raises(BLUESTError):
            _toy(F, SamplingMixin, B, weights=bad).get_models_inner_products()
    for name in ("reorder_graph_nodes", "reorder_all_graph_nodes"):
        with pytest.raises(BLUESTError):
            getattr(p, name)()
    with pytest.raises(BLUESTError):                                    # sample files stay refused
        _toy(F, PM, B, weights=[None, w], samplefile="samples.npz")
    with pytest.raises(BLUESTError):                                    # no SamplingMixin: variance_test stays refused
        _toy(F, PM, B, weights=[None, w]).variance_test(eps=0.1)


def test_a_width_mismatch_is_refused():
    from bluest_amd.fields import draw_field_values
    from bluest_amd.sap import BLUESTError
    F, PM, B = _classes()
    p = _toy(F, B, weights=[None, np.ones(3)], sample_batch_size=4)
    p.evaluate = lambda ls, samples, N=1: [[np.zeros(4) for _ in ls], [np.zeros((4, 2)) for _ in ls]]
    with pytest.raises(BLUESTError, match="declares 3"):
        draw_field_values(p, [0, 1], 4, [1, 3])
    p.evaluate = lambda ls, samples, N=1: [[np.zeros(4) for _ in ls], [np.zeros((3, 4)) for _ in ls]]     # 12 values, wrong way round
    with pytest.raises(BLUESTError, match="declares 3"):
        draw_field_values(p, [0, 1], 4, [1, 3])
    p.evaluate = lambda ls, samples, N=1: [[np.zeros(4) for _ in ls], [np.arange(12.0).reshape(4, 3) + l for l in ls]]
    assert draw_field_values(p, [0, 1], 4, [1, 3])[1].shape == (4, 2, 3)
    with pytest.raises(BLUESTError, match="batch of 2"):                # batches of 4 and 2: the second one comes back with 4 rows
        draw_field_values(p, [0, 1], 6, [1, 3])


def test_drawing_keeps_the_call_sequence_and_shapes():
    from bluest_amd.fields import draw_field_values
    F, PM, B = _classes()
    p = _toy(F, B, weights=[None, np.ones(3)], sample_batch_size=4)
    seen = []

    def sampler(ls, N=1):
        seen.append((list(ls), N))
        return [np.full(N, float(len(seen)))] * len(ls)
    p.sampler = sampler
    bad = [True]

    def evaluate(ls, samples, N=1):
        k = samples[0]
        field = [k[:, None] * np.array([1.0, 10.0, 100.0]) + l for l in ls]
        if bad and len(seen) == 2:
            bad.pop()
            field[0][0, 1] = np.nan                                     # a non-finite batch is drawn again
        return [[k + l for l in ls], field]
    p.evaluate = evaluate
    scalar, field = draw_field_values(p, [0, 1], 6, [1, 3])
    assert seen == [([0, 1], 4), ([0, 1], 2), ([0, 1], 2)]
    assert scalar.shape == (6, 2, 1) and field.shape == (6, 2, 3)
    assert np.array_equal(scalar[:, 1, 0], [2.0] * 4 + [4.0] * 2) and np.array_equal(field[5, 1], [4.0, 31.0, 301.0])


def test_without_a_gpu_the_calls_raise():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bluest_amd import _lib, fields
    with pytest.raises(_lib.BluestHipError):
        fields.field_statistics(np.ones((4, 2, 3)), np.ones(3))
    with pytest.raises(_lib.BluestHipError):
        fields.field_group_sums([np.ones((4, 2, 3))])
    with pytest.raises(ValueError):
        fields.field_statistics(np.ones((4, 2, 3)), np.ones(2))


def test_the_samples_are_split_over_the_ranks_and_gathered_on_rank_0(monkeypatch):
    from bluest_amd import fields
    from bluest_amd.estimator import SamplingMixin
    from test_estimator_host import FakeComm
    F, PM, B = _classes()
    seen = []

    def sums(values, **kw):
        seen.append(values)
        return fields_ref.field_group_sums(values, **kw)
    monkeypatch.setattr(fields, "field_group_sums", sums)

    class P(F, SamplingMixin, B):
        def output_weights(self): return [None, np.array([1.0, 2.0])]

        def sampler(self, ls, N=1):
            self.asked.append(N)
            return [100.0 * self.mpiRank + np.arange(N)] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[s + l for s, l in zip(samples, ls)], [np.stack([s, -s], axis=1) for s in samples]]

    board, size, results = {}, 3, {}
    C = [np.eye(2) + 0.5] * 2
    for rank in (2, 1, 0):                                              # rank 0 last: it finds the others' shares gathered
        p = P(2, C=C, costs=np.array([2.0, 1.0]), n_outputs=2, verbose=False, sample_batch_size=3, comm=FakeComm(rank, size, board))
        p.asked = []
        results[rank] = (p._group_sums([0, 1], 11), p.asked)
    assert [results[r][1] for r in range(3)] == [[3, 1], [3, 1], [3]]  # 11 = 4 + 4 + 3, in batches of 3
    assert len(seen) == 2 and [v[0].shape for v in seen] == [(11, 2, 1), (11, 2, 2)]       # rank 0 alone, one call per output
    assert seen[1][0][:, 0, 0].tolist() == [0, 1, 2, 0, 100, 101, 102, 100, 200, 201, 202]   # rank order, each rank in batches
    number, field = results[0][0]
    assert number == [float(seen[0][0][:, 0, 0].sum()), float(seen[0][0][:, 1, 0].sum())]
    assert np.array_equal(field[0], seen[1][0][:, 0].sum(axis=0)) and field[0][1] == -field[0][0]

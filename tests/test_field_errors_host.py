"""
Host tests of bluest_amd.field_errors: the build and the binding of bluest_field_weighted_moments, the argument checks of
field_weighted_moments, the numpy restatement of Part 15 (tests/field_moments_ref.py) against long-double sums, and FieldErrorsMixin
with the restatements standing in for both kernels on a seeded problem with one number and one field per model: the sampler is
called as FieldOutputsMixin calls it and solve() returns its bits, field_sample_moments holds every sampled group, the error bars
in the norm and per component are the formulas recomputed with numpy alone on the same draws, the refusals are in place, and the
sampled variance is unbiased under a wrong model covariance.  The allocation and the weights are set by hand here
(tests/test_gpu_field_errors.py runs the real ones).
"""
import ctypes

import numpy as np
import pytest

import field_moments_ref as ref
import fields_ref
import gsums_ref
from gsums_ref import same_bits
from test_estimator_host import FakeComm

U = gsums_ref.U
M, D = 3, 4
MASS = np.array([0.5, 1.0, 2.0, 0.25])
AMP = np.array([1.0, -0.5, 2.0, 0.1])
GROUPS = [[0, 1, 2], [0, 1], [1, 2], [2], [0, 2], [1]]
SAMPLES = np.array([9, 0, 40, 150, 1, 5])                               # group 1 is not drawn, group 4 is drawn once


def _bases():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_errors import FieldErrorsMixin
    from bluest_amd.fields import FieldOutputsMixin
    return FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem


@pytest.fixture
def stubbed(monkeypatch):
    """field_group_sums and field_weighted_moments -> their restatements; every field_weighted_moments call is kept"""
    from bluest_amd import field_errors, fields
    seen = []

    def fake_moments(values, coef, slab_bytes=None):
        seen.append((values, np.array(coef)))
        return ref.field_weighted_moments(values, coef)
    monkeypatch.setattr(fields, "field_group_sums", lambda values, **kw: fields_ref.field_group_sums(values, **kw))
    monkeypatch.setattr(field_errors, "field_weighted_moments", fake_moments)
    return seen


def model_covariances():
    A = np.array([[1.0, 0.6, 0.3], [0.6, 1.2, 0.5], [0.3, 0.5, 0.9]])
    return [A, float(np.dot(AMP * MASS, AMP)) * A]


def toy(*bases, seed=3, comm=None, batch=16):
    """one number and one field of D components per model, drawn in batches; evaluate records what it returns"""
    class Toy(*bases):
        def output_weights(self): return [None, MASS]

        def sampler(self, ls, N=1):
            self.calls.append((list(ls), int(N)))
            z = self.rng.randn(int(N), 1 + len(ls))
            return [(z[:, 0], z[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            y = [2.0 + 0.8 ** l * s[0] + 0.3 * (l + 1) * s[1] for l, s in zip(ls, samples)]      # [N2] per model
            Ps = [y, [AMP[None, :] * v[:, None] + np.arange(D)[None, :] for v in y]]
            self.drawn.append((list(ls), Ps))
            return Ps

    kw = dict(C=model_covariances(), costs=np.array([4.0, 2.0, 1.0]), n_outputs=2, verbose=False, sample_batch_size=batch)
    if comm is not None:
        kw["comm"] = comm
    p = Toy(M, **kw)
    p.rng, p.calls, p.drawn = np.random.RandomState(seed), [], []
    return p


def hand_set(p, seed=5):
    """the allocation in place of setup_solver, and random weights in place of the GPU solve; output 1 does not see group 5"""
    chosen = np.flatnonzero(SAMPLES > 0)
    T = sum(len(GROUPS[g]) for g in chosen)
    W = np.random.RandomState(seed).randn(2, T)
    W[1, T - 1:] = 0.0                                                  # group 5 = [1], the last column
    Vs = np.array([0.04, 0.09])
    out = {"budget": None, "eps": [0.2, 0.3], "samples": SAMPLES, "flattened_groups": GROUPS, "variances": Vs, "cost": 7.0}
    p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (W, Vs))
    return W


def segments_drawn(p):
    """per sampled group (in list order) and output the values [N, L, d_n] of the first estimator that p drew"""
    segs, k = [], 0
    for g in np.flatnonzero(SAMPLES > 0).tolist():
        need, number, field = int(SAMPLES[g]), [], []
        while need > 0:
            ls, Ps = p.drawn[k]
            assert ls == GROUPS[g]
            number.append(np.stack(Ps[0], axis=1)[:, :, None])
            field.append(np.stack(Ps[1], axis=1))
            need -= len(Ps[0][0])
            k += 1
        assert need == 0
        segs.append((g, [np.concatenate(number), np.concatenate(field)]))
    return segs, k


def numpy_errors(p, W, segs):
    """the formulas, from numpy alone: per output the sampled variance in the norm, the map, the unsampled share and per group
    the variance of z"""
    weights = [np.ones(1), MASS]
    norm, maps, unsampled, per_group = np.zeros(2), [np.zeros(1), np.zeros(D)], [0.0, 0.0], [{}, {}]
    c = 0
    for g, vals in segs:
        ls, m = GROUPS[g], int(SAMPLES[g])
        for n in range(2):
            w = W[n, c:c + len(ls)]
            z = np.einsum("j,ijc->ic", w, vals[n])
            var = z.var(axis=0, ddof=1) if m >= 2 else np.full(z.shape[1], np.nan)
            per_group[n][g] = (m, var)
            if not w.any():
                continue
            if m >= 2:
                norm[n] += m * float(np.dot(weights[n], var))
                maps[n] += m * var
            else:
                share = m * float(w @ p.get_covariance(n)[np.ix_(ls, ls)] @ w)
                norm[n] += share
                unsampled[n] += share
        c += len(ls)
    return np.sqrt(norm), [np.sqrt(a) for a in maps], unsampled, per_group


# ---- the build and the binding ----------------------------------------------------------------------------------------------------
def test_the_unit_is_built_and_the_symbol_bound():
    from bluest_amd import _lib, build
    assert "field_moments.hip" in build.SOURCES
    build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bluest_field_weighted_moments")
    assert len(_lib.SIGNATURES["bluest_field_weighted_moments"]) == 9
    assert _lib.lib().bluest_field_weighted_moments.argtypes == _lib.SIGNATURES["bluest_field_weighted_moments"]
    assert _lib.lib().bluest_abi_version() == 1


def test_field_weighted_moments_checks_its_arguments():
    import torch
    from bluest_amd import field_errors
    with pytest.raises(ValueError):
        field_errors.field_weighted_moments([], [])
    with pytest.raises(ValueError):
        field_errors.field_weighted_moments([np.ones((4, 2, 3)), np.ones((4, 2, 2))], np.ones(4))      # two widths
    with pytest.raises(ValueError):
        field_errors.field_weighted_moments([np.ones((4, 2))], np.ones(2))
    with pytest.raises(ValueError):
        field_errors.field_weighted_moments([torch.ones(4, 2, 3, dtype=torch.float32)], np.ones(2))
    with pytest.raises(ValueError):
        field_errors.field_weighted_moments([np.ones((4, 2, 3))], np.ones(3))                            # one entry per column
    with pytest.raises(ValueError):
        field_errors.field_weighted_moments([np.ones((4, 2, 3))], np.array([1.0, np.inf]))


def test_the_arguments_are_checked_first_and_there_is_no_cpu_path():
    import torch
    from bluest_amd import _lib, field_errors
    v, coef = np.ones((4, 2, 3)), np.ones(2)
    zsum, zsq = np.full((1, 3), -7.0), np.full((1, 3), -7.0)
    ptrs = (ctypes.c_void_p * 1)(_lib.ptr(v))
    counts, sizes = np.array([4], dtype=np.int64), np.array([2], dtype=np.int32)
    call = lambda S, c: _lib.lib().bluest_field_weighted_moments(S, 3, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                                                 _lib.ptr(c), _lib.ptr(zsum), _lib.ptr(zsq), None)
    assert call(0, coef) == 1 and call(1, np.array([1.0, np.nan])) == 1 and call(1, None) == 1
    assert (zsum == -7.0).all() and (zsq == -7.0).all()
    if not torch.cuda.is_available():
        assert call(1, coef) == 3 and (zsum == -7.0).all() and (zsq == -7.0).all()      # BLUEST_ERR_NOGPU, nothing written
        with pytest.raises(_lib.BluestHipError):
            field_errors.field_weighted_moments([v], coef)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(1, 2, 3), (2, 3, 2), (17, 5, 3), (129, 4, 2), (300, 2, 5), (40, 33, 1)])
def test_the_restatement_is_inside_the_rounding_bound(shape):
    N, L, d = shape
    rng = np.random.RandomState(sum(shape))
    v = 1.5 + 10.0 ** rng.uniform(-3, 3, L)[None, :, None] * rng.randn(N, L, d)
    c = rng.randn(L)
    zsum, zsq = ref.segment_moments(v, c)
    s1, s2, b1, b2 = ref.moments_ld(v, c)
    assert (np.abs(zsum.astype(gsums_ref.LD) - s1) <= b1).all() and (np.abs(zsq.astype(gsums_ref.LD) - s2) <= b2).all()
    if N == 1:
        assert (zsum == 0).all() and (zsq == 0).all() and not np.signbit(zsum).any() and not np.signbit(zsq).any()
    else:
        z = np.einsum("j,ijc->ic", c, v)
        assert np.allclose(ref.variance_of(N, zsum, zsq), z.var(axis=0, ddof=1), rtol=1e-9)


def test_exact_chains_take_the_fast_path_to_the_same_bits():
    """on data26 q + a * b has the bits of the fma: the restatement's two forms agree, and the order of the additions still shows
    (the plain long-double sum of squares differs in some entries)"""
    for signed in (False, True):
        v, c = ref.data26(150, 5, 3, 3, signed=signed)
        slow, fast = ref.segment_moments(v, c), ref.segment_moments(v, c, exact_products=True)
        assert same_bits(slow[0], fast[0]) and same_bits(slow[1], fast[1])
        if not signed:
            assert (fast[1] != ref.moments_ld(v, c)[1].astype(np.float64)).any()
            z = ref.chains(v, c, exact_products=True)
            assert np.abs(z[1:]).min() * 2.0 ** 30 >= 2.0 ** 24        # (scaled by at most 2^-30: z is of the order 2^25)
    rng = np.random.RandomState(1)
    with pytest.raises(AssertionError):
        ref.segment_moments(rng.randn(9, 3, 2), rng.randn(3), exact_products=True)


# ---- the mix-in -------------------------------------------------------------------------------------------------------------------
def test_solve_replays_the_call_sequence_and_keeps_the_moments(stubbed):
    from bluest_amd.sap import BLUESTError
    FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem = _bases()
    plain = toy(FieldOutputsMixin, SamplingMixin, BLUEProblem)
    hand_set(plain)
    want = plain.solve(K=3, eps=[0.2, 0.3])
    assert not stubbed                                                  # without the new mix-in nothing changes
    p = toy(FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem)
    for method in (p.sampled_errors, p.sampled_error_fields):
        with pytest.raises(BLUESTError):
            method()                                                    # before a solve()
    W = hand_set(p)
    mus, errs, cost = p.solve(K=3, eps=[0.2, 0.3])
    assert p.calls == plain.calls and len(p.calls) == sum(-(-int(m) // 16) for m in SAMPLES)
    assert isinstance(mus[0], float) and same_bits(mus[0], want[0][0]) and same_bits(mus[1], want[0][1])
    assert same_bits(errs, want[1]) and cost == want[2]
    segs, n_calls = segments_drawn(p)
    chosen = np.flatnonzero(SAMPLES > 0).tolist()
    assert len(stubbed) == 2                                            # one flush: ONE call per output
    for n, (values, coef) in enumerate(stubbed):
        assert [v.shape for v in values] == [(int(SAMPLES[g]), len(GROUPS[g]), (1, D)[n]) for g in chosen]
        assert np.array_equal(coef, W[n]) and all(np.array_equal(v, s[1][n]) for v, s in zip(values, segs))
    want_errs, want_maps, want_unsampled, per_group = numpy_errors(p, W, segs)
    for n in range(2):
        assert sorted(p.field_sample_moments[n]) == chosen
        for g in chosen:
            N, var = p.field_sample_moments[n][g]
            assert N == int(SAMPLES[g]) and var.shape == ((1, D)[n],)
            assert np.allclose(var, per_group[n][g][1], rtol=1e-10, atol=0, equal_nan=True) and np.isnan(var).all() == (N < 2)
    assert np.allclose(p.sampled_errors(), want_errs, rtol=1e-10, atol=0)
    assert np.allclose(p.sampled_errors(source="model"), errs, rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        p.sampled_errors(source="pilot")
    maps, unsampled = p.sampled_error_fields()
    assert isinstance(maps[0], float) and maps[1].shape == (D,)
    assert np.allclose(maps[0], want_maps[0][0], rtol=1e-10) and np.allclose(maps[1], want_maps[1], rtol=1e-10, atol=0)
    assert np.allclose(unsampled, want_unsampled, rtol=1e-10, atol=0) and unsampled[0] > 0 and unsampled[1] > 0
    # the map and the unsampled share make up the error in the norm
    for n, w in enumerate((np.ones(1), MASS)):
        assert np.isclose(np.dot(w, np.atleast_1d(maps[n]) ** 2) + unsampled[n], p.sampled_errors()[n] ** 2, rtol=1e-12)
    # a variance test's repeats are not looked at, and leave the moments of the solve alone
    before = [dict(m) for m in p.field_sample_moments]
    p.variance_test(eps=[0.2, 0.3], K=3, N=2)
    assert len(stubbed) == 2 and all(sorted(a) == sorted(b) for a, b in zip(p.field_sample_moments, before))
    assert all(a[g][1] is b[g][1] for a, b in zip(p.field_sample_moments, before) for g in chosen)


def test_every_flush_brings_its_own_weights(stubbed, monkeypatch):
    """with a flush after every group the moments are the same, from ONE call per output and flush"""
    from bluest_amd import fields
    bases = _bases()
    p, q = toy(*bases), toy(*bases)
    W = hand_set(p)
    hand_set(q)
    p.solve(K=3, eps=[0.2, 0.3])
    whole = list(stubbed)
    del stubbed[:]
    monkeypatch.setattr(fields, "SLAB_BYTES", 1)
    q.solve(K=3, eps=[0.2, 0.3])
    chosen = np.flatnonzero(SAMPLES > 0).tolist()
    assert len(whole) == 2 and len(stubbed) == 2 * len(chosen)
    col = 0
    for i, g in enumerate(chosen):
        for n in range(2):
            values, coef = stubbed[2 * i + n]
            assert len(values) == 1 and np.array_equal(coef, W[n, col:col + len(GROUPS[g])])
            assert same_bits(q.field_sample_moments[n][g][1], p.field_sample_moments[n][g][1])
        col += len(GROUPS[g])


def test_the_moments_are_taken_on_rank_0_after_the_gather(stubbed):
    bases = _bases()

    class P(*bases):
        def output_weights(self): return [None, np.array([1.0, 2.0])]

        def sampler(self, ls, N=1):
            return [100.0 * self.mpiRank + np.arange(N)] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[s * (1 + l) for s, l in zip(samples, ls)], [np.stack([s, -s * (1 + l)], axis=1) for s, l in zip(samples, ls)]]

    board, size, results = {}, 3, {}
    samples, groups = np.array([0, 7, 4]), [[0], [0, 1], [1]]
    W = np.array([[1.0, 1.0, 1.0], [0.5, 2.0, 1.0]])
    for rank in (2, 1, 0):                                              # rank 0 last: it finds the others' shares gathered
        p = P(2, C=[np.eye(2) + 0.5] * 2, costs=np.array([2.0, 1.0]), n_outputs=2, verbose=False, sample_batch_size=3,
              comm=FakeComm(rank, size, board))
        out = {"budget": None, "eps": [0.1, 0.1], "samples": samples, "flattened_groups": groups, "variances": np.ones(2), "cost": 1.0}
        p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (W, np.ones(2)))
        p._collecting_fields = [{}, {}]                                 # what solve() does around the draw (the ranks of this
        p._sample_estimators(1)                                         # board run one after the other: no broadcast to wait for)
        results[rank] = p._collecting_fields
    assert len(stubbed) == 2                                            # the kernel runs on rank 0 alone, once per output
    assert [v.shape for v in stubbed[0][0]] == [(7, 2, 1), (4, 1, 1)] and [v.shape for v in stubbed[1][0]] == [(7, 2, 2), (4, 1, 2)]
    col = stubbed[0][0][0][:, 0, 0]
    assert col.tolist() == [0, 1, 2, 100, 101, 200, 201]               # 7 = 3 + 2 + 2, in rank order
    assert results[1] == [{}, {}] and results[2] == [{}, {}] and sorted(results[0][0]) == [1, 2] and results[0][1][1][0] == 7
    assert np.allclose(results[0][0][1][1], np.var(col + 2 * col, ddof=1), rtol=1e-12)
    assert np.allclose(results[0][1][1][1], [np.var(0.5 * col + 2.0 * col, ddof=1), np.var(-0.5 * col - 4.0 * col, ddof=1)], rtol=1e-12)


def test_what_is_refused(stubbed):
    from bluest_amd.sap import BLUESTError
    FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem = _bases()
    kw = dict(C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False)
    q = type("Q", (FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem), {})(2, **kw)
    for refused in (q.reorder_graph_nodes, q.reorder_all_graph_nodes):
        with pytest.raises(BLUESTError):
            refused()
    from bluest_amd.pilot import PilotMixin
    with pytest.raises(BLUESTError):                                    # sample files stay refused (PilotMixin is where they would be read)
        type("S", (FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, PilotMixin, BLUEProblem), {})(2, samplefile="samples.npz", **kw)

    class Inner(FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem):
        def get_models_inner_products(self):
            return [lambda a, b: float(np.dot(a, b))]

    class NoSampling(FieldErrorsMixin, FieldOutputsMixin, BLUEProblem):
        pass

    for cls in (Inner, NoSampling):
        p = cls(2, **kw)
        taken = []
        orig = FieldOutputsMixin.solve
        try:
            FieldOutputsMixin.solve = lambda self, **a: taken.append(sorted(a)) or "parent"
            assert p.solve(eps=0.1) == "parent" and len(taken) == 1 and "optimization_solver_params" in taken[0]
        finally:
            FieldOutputsMixin.solve = orig
        assert p.field_sample_moments is None
        p.field_sample_moments, p.MOSAP_output = [{}], {}
        for method in (p.sampled_errors, p.sampled_error_fields):
            with pytest.raises(BLUESTError):
                method()
    assert not stubbed
    assert not hasattr(FieldErrorsMixin, "variance_test") and not hasattr(FieldErrorsMixin, "complexity_test")     # inherited untouched


# ---- the formula is unbiased -----------------------------------------------------------------------------------------------------
def test_the_sampled_variance_is_unbiased_under_a_wrong_model_covariance(monkeypatch):
    """Three models with a field of three components each, the groups {0,1,2}, {1,2}, {2} drawn 12, 40 and 150 times; component c
    of model l is s_c times a draw from C_true, while the weights come from a model covariance with smaller variances and stronger
    correlations.  Over R = 400 independent solves the mean of sampled_errors()^2 must lie within 5 of its own standard errors of
    the estimator's true variance in the norm, sum_c w_c s_c^2 sum_g m_g u' C_true u -- which the model's promise misses by far
    more -- and the mean of every component of the squared map within 5 standard errors of s_c^2 sum_g m_g u' C_true u.  numpy
    stands in for the kernels: this is about the formulas."""
    from bluest_amd import field_errors, fields
    bases = _bases()
    C_model = np.array([[1.0, 0.6, 0.3], [0.6, 1.2, 0.5], [0.3, 0.5, 0.9]])
    C_true = np.array([[2.5, 1.0, 0.4], [1.0, 2.0, 0.6], [0.4, 0.6, 2.2]])
    scale, mass = np.array([1.0, 0.5, 2.0]), np.array([0.5, 2.0, 1.0])
    groups, m = [[0, 1, 2], [1, 2], [2]], np.array([12, 40, 150])
    Phi = np.zeros((3, 3))
    for ls, mg in zip(groups, m):
        Phi[np.ix_(ls, ls)] += mg * np.linalg.inv(C_model[np.ix_(ls, ls)])
    v = np.linalg.inv(Phi)[0]
    W = np.concatenate([np.linalg.inv(C_model[np.ix_(ls, ls)]) @ v[ls] for ls in groups])[None, :]
    true_1d = sum(mg * w @ C_true[np.ix_(ls, ls)] @ w for ls, mg, w in zip(groups, m, np.split(W[0], [3, 5])))
    true_map = scale ** 2 * true_1d
    true_var = float(np.dot(mass, true_map))
    promised = float(np.dot(mass, scale ** 2)) * float(np.linalg.inv(Phi)[0, 0])

    def numpy_moments(values, coef, slab_bytes=None):
        out, c = [], 0
        for y in values:
            z = np.einsum("j,ijc->ic", coef[c:c + y.shape[1]], y - y[:1])
            out.append((y.shape[0], z.sum(axis=0), (z * z).sum(axis=0)))
            c += y.shape[1]
        return out

    def numpy_sums(values, weights=None, repeat_of=None, R=None, slab_bytes=None):
        sums = [y.sum(axis=0) for y in values]
        return sums, (np.asarray(weights)[:, None] * np.concatenate(sums, axis=0)).sum(axis=0)[None, :]
    monkeypatch.setattr(field_errors, "field_weighted_moments", numpy_moments)
    monkeypatch.setattr(fields, "field_group_sums", numpy_sums)

    class Toy(*bases):
        def output_weights(self): return [mass]

        def sampler(self, ls, N=1):
            z = self.rng.multivariate_normal(np.zeros(len(ls)), C_true[np.ix_(ls, ls)], size=N)
            return [z[:, i] for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            return [[2.0 + scale[None, :] * s[:, None] for s in samples]]

    p = Toy(3, C=float(np.dot(mass, scale ** 2)) * C_model, costs=np.array([4.0, 2.0, 1.0]), verbose=False, sample_batch_size=64)
    p.rng = np.random.RandomState(2024)
    out = {"budget": None, "eps": [0.1], "samples": m, "flattened_groups": groups, "variances": np.array([promised]), "cost": 1.0}
    p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (W, np.array([promised])))
    R, est, maps, mus = 400, [], [], []
    for _ in range(R):
        mu, errs, _ = p.solve(eps=0.1)
        mus.append(mu[0])
        est.append(p.sampled_errors()[0] ** 2)
        fmap, unsampled = p.sampled_error_fields()
        assert unsampled == [0.0]
        maps.append(fmap[0] ** 2)
    est, maps, mus = np.array(est), np.array(maps), np.array(mus)
    se, se_map = est.std(ddof=1) / np.sqrt(R), maps.std(axis=0, ddof=1) / np.sqrt(R)
    print("true variance", true_var, "mean of the sampled variances", est.mean(), "+-", se, "promised by the model", promised)
    print("true map", true_map, "mean of the sampled maps", maps.mean(axis=0), "+-", se_map, "variances of the", R, "estimates", mus.var(axis=0, ddof=1))
    assert abs(est.mean() - true_var) <= 5 * se
    assert (np.abs(maps.mean(axis=0) - true_map) <= 5 * se_map).all()
    assert abs(promised - true_var) > 20 * se                           # the model's promise is not the truth here
    assert np.isclose(p.sampled_errors(source="model")[0] ** 2, promised, rtol=1e-12)
    assert (np.abs(mus.var(axis=0, ddof=1) / true_map - 1) < 5 * np.sqrt(2.0 / (R - 1))).all()    # and the truth is what the estimates show

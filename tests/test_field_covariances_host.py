"""
Host tests of bluest_amd.field_covariances: the build and the binding of bluest_field_group_moments, its argument checks (every
BLUEST_ERR_ARG before an output byte is written), the numpy restatement of Part 16 (tests/field_cov_ref.py) against its anchors in
Parts 13 and 15 and against long-double sums, and FieldCovariancesMixin with the restatements standing in for the kernels on the
seeded problem of tests/test_field_errors_host.py: the sampler is called as FieldOutputsMixin calls it and solve() returns its bits,
field_sample_covariances holds every sampled group, the error bars and the pooled covariances are the formulas recomputed with
numpy alone on the same draws, the hook chains in front of FieldErrorsMixin, and the refusals are in place.
"""
import ctypes
import types

import numpy as np
import pytest

import field_cov_ref as ref
import field_moments_ref
import fields_ref
import gsums_ref
import moments_ref
from gsums_ref import LD, U, same_bits
from test_field_errors_host import D, GROUPS, MASS, SAMPLES, hand_set, segments_drawn, toy


def _bases(errors=False):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_covariances import FieldCovariancesMixin
    from bluest_amd.field_errors import FieldErrorsMixin
    from bluest_amd.fields import FieldOutputsMixin
    return (FieldCovariancesMixin,) + ((FieldErrorsMixin,) if errors else ()) + (FieldOutputsMixin, SamplingMixin, BLUEProblem)


@pytest.fixture
def stubbed(monkeypatch):
    """field_group_sums, field_group_moments and field_weighted_moments -> their restatements; the calls of the last two are kept"""
    from bluest_amd import field_covariances, field_errors, fields
    seen = {"cov": [], "err": []}

    def fake_cov(values, w, with_first=False, slab_bytes=None):
        seen["cov"].append((values, np.array(w)))
        return ref.field_group_moments(values, w, with_first=with_first)

    def fake_err(values, coef, slab_bytes=None):
        seen["err"].append((values, np.array(coef)))
        return field_moments_ref.field_weighted_moments(values, coef)
    monkeypatch.setattr(fields, "field_group_sums", lambda values, **kw: fields_ref.field_group_sums(values, **kw))
    monkeypatch.setattr(field_covariances, "field_group_moments", fake_cov)
    monkeypatch.setattr(field_errors, "field_weighted_moments", fake_err)
    return seen


# ---- the build and the binding ----------------------------------------------------------------------------------------------------
def test_the_unit_is_built_and_the_symbol_bound():
    from bluest_amd import _lib, build
    assert "field_cov.hip" in build.SOURCES and "field_cov.hip" not in build.SOURCE_FLAGS
    build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bluest_field_group_moments")
    assert len(_lib.SIGNATURES["bluest_field_group_moments"]) == 10
    assert _lib.lib().bluest_field_group_moments.argtypes == _lib.SIGNATURES["bluest_field_group_moments"]
    assert _lib.lib().bluest_abi_version() == 1


def test_field_group_moments_checks_its_arguments():
    import torch
    from bluest_amd import field_covariances as fc
    with pytest.raises(ValueError):
        fc.field_group_moments([], np.ones(3))
    with pytest.raises(ValueError):
        fc.field_group_moments([np.ones((4, 2, 3)), np.ones((4, 2, 2))], np.ones(3))       # two widths
    with pytest.raises(ValueError):
        fc.field_group_moments([np.ones((4, 2))], np.ones(2))
    with pytest.raises(ValueError):
        fc.field_group_moments([torch.ones(4, 2, 3, dtype=torch.float32)], np.ones(3))
    with pytest.raises(ValueError):
        fc.field_group_moments([np.ones((4, 2, 3))], np.ones(2))                             # one weight per component
    for bad in (np.inf, np.nan, -1.0):
        with pytest.raises(ValueError):
            fc.field_group_moments([np.ones((4, 2, 3))], np.array([1.0, bad, 1.0]))
    assert np.isnan(fc.covariance_of(1, np.zeros((2, 2)), np.zeros((2, 2)))).all()
    assert fc.covariance_of(3, np.full((1, 1), 8.0), np.full((1, 1), 6.0))[0, 0] == 3.0


def _call(S, d, counts, sizes, ptrs, w, second, cross, first):
    from bluest_amd import _lib
    return _lib.lib().bluest_field_group_moments(S, d, _lib.ptr(counts), _lib.ptr(sizes), None if ptrs is None else ctypes.cast(ptrs, ctypes.c_void_p),
                                                 _lib.ptr(w), _lib.ptr(second), _lib.ptr(cross), _lib.ptr(first), None)


def test_every_argument_error_comes_before_anything_is_written_and_there_is_no_cpu_path():
    import torch
    from bluest_amd import _lib, field_covariances as fc
    v, w = np.ones((4, 2, 3)), np.ones(3)
    second, cross, first = np.full(3, -7.0), np.full(3, -7.0), np.full((2, 3), -7.0)
    ptrs = (ctypes.c_void_p * 1)(_lib.ptr(v))
    counts, sizes = np.array([4], dtype=np.int64), np.array([2], dtype=np.int32)
    good = dict(S=1, d=3, counts=counts, sizes=sizes, ptrs=ptrs, w=w, second=second, cross=cross, first=first)
    bad = [dict(S=0), dict(d=0), dict(counts=None), dict(sizes=None), dict(ptrs=None), dict(w=None), dict(second=None), dict(cross=None),
           dict(sizes=np.array([0], dtype=np.int32)), dict(sizes=np.array([65], dtype=np.int32)), dict(counts=np.array([-1], dtype=np.int64)),
           dict(ptrs=(ctypes.c_void_p * 1)(None)), dict(ptrs=(ctypes.c_void_p * 1)(_lib.ptr(v) + 4)),
           dict(w=np.array([1.0, np.nan, 1.0])), dict(w=np.array([1.0, np.inf, 1.0])), dict(w=np.array([1.0, -0.5, 1.0]))]
    for change in bad:
        assert _call(**dict(good, **change)) == 1, change
        assert (second == -7.0).all() and (cross == -7.0).all() and (first == -7.0).all(), change
    assert _call(**dict(good, counts=np.array([0], dtype=np.int64), ptrs=(ctypes.c_void_p * 1)(None))) in (0, 3)      # null is fine without samples
    second[:], cross[:], first[:] = -7.0, -7.0, -7.0
    # the 2^31 limits, with counts nobody could store: the checks come before any pointer is followed
    big = lambda n, L: (np.array([n], dtype=np.int64), np.array([L], dtype=np.int32))
    c, s = big(128 * 2 ** 31, 1)                                        # chunks
    assert _call(**dict(good, d=1, counts=c, sizes=s)) == 1
    c, s = big(4, 64)                                                   # column-components T d
    assert _call(**dict(good, d=2 ** 25, counts=c, sizes=s)) == 1
    c, s = big(128 * 2 ** 21, 64)                                       # partial sums: 2^21 chunks x 2080 pairs x 1 tile
    assert _call(**dict(good, d=1, counts=c, sizes=s)) == 1
    c, s = big(128 * 2 ** 23, 64)                                       # partial sums of f: 2^23 chunks x 8 classes x 64 columns
    assert _call(**dict(good, d=1, counts=c, sizes=s)) == 1
    S = 2 ** 31 // 2080 + 1                                             # packed pairs: S triangles of 2080
    many = (ctypes.c_void_p * S)()
    assert _call(**dict(good, S=S, d=1, counts=np.zeros(S, dtype=np.int64), sizes=np.full(S, 64, dtype=np.int32), ptrs=many)) == 1
    assert b"packed pairs" in _lib.lib().bluest_last_error()
    assert (second == -7.0).all() and (cross == -7.0).all() and (first == -7.0).all()
    if not torch.cuda.is_available():
        assert _call(**good) == 3 and (second == -7.0).all() and (cross == -7.0).all() and (first == -7.0).all()     # BLUEST_ERR_NOGPU
        with pytest.raises(_lib.BluestHipError):
            fc.field_group_moments([v], w)


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def test_the_fma_of_the_c_library_is_the_exact_one():
    rng = np.random.RandomState(0)
    a, b = rng.randn(2000), rng.randn(2000)
    c = -(a * b) * (1 + rng.choice([0.0, 2.0 ** -52, -2.0 ** -52, 1e-3], size=2000))       # cancellation: the rounding of a * b shows
    a[:3], b[:3], c[:3] = [1 + 2.0 ** -52, 3.0, 2.0 ** 53], [1 + 2.0 ** -52, 2.0 ** -53, 1.0], [-1.0, 1.0, 2.0 ** -53]    # ties among them
    assert same_bits(ref._fma(a, b, c).astype(np.float64), ref._fma_c(a, b, c).astype(np.float64))
    assert (ref._fma(a, b, c).astype(np.float64) != a * b + c).any()


@pytest.mark.parametrize("N,L", [(0, 2), (1, 3), (2, 1), (17, 3), (129, 4), (300, 2)])
def test_at_one_component_and_weight_one_it_is_part_13(N, L):
    v = 3.0 + np.random.RandomState(N + L).randn(N, L, 1)
    first, second, cross = ref.segment_moments(v, [1.0])
    want_first, want_second = moments_ref.segment_moments(v[None, :, :, 0])
    assert same_bits(first[:, 0], want_first[0]) and same_bits(second, want_second[0])
    j, k = np.triu_indices(L)
    assert same_bits(cross, first[j, 0] * first[k, 0])                  # one fma from +0.0, the join adds +0.0
    v26 = moments_ref.data26(1, max(N, 1), L, 4)[0][:, :, None]
    fast, slow = ref.segment_moments(v26, [1.0], exact_products=True), ref.segment_moments(v26, [1.0])
    assert all(same_bits(a, b) for a, b in zip(fast, slow))


@pytest.mark.parametrize("N,d,c", [(1, 3, 0), (40, 9, 8), (130, 9, 3), (300, 17, 16)])
def test_one_model_and_a_one_hot_weight_are_part_15(N, d, c):
    v = 1.5 + np.random.RandomState(N + d).randn(N, 1, d)
    w = np.zeros(d)
    w[c] = 1.0
    first, second, cross = ref.segment_moments(v, w)
    zsum, zsq = field_moments_ref.segment_moments(v, [1.0])
    assert same_bits(first[0], zsum) and same_bits(second, zsq[c:c + 1])
    assert same_bits(cross, first[0, c:c + 1] ** 2)


@pytest.mark.parametrize("shape", [(2, 1, 1), (3, 2, 9), (17, 5, 3), (129, 4, 2), (300, 2, 5), (40, 9, 17), (5, 3, 600)])
def test_the_restatement_is_inside_the_rounding_bound(shape):
    """second, cross and f against long-double sums of the same d, and the covariance they imply against a two-pass long-double
    covariance of the values themselves: the shift d = fl(y - y_0) adds a relative error u per value, 2 u per product, on top of
    the bounds of field_cov_ref.moments_ld"""
    N, L, d = shape
    rng = np.random.RandomState(sum(shape))
    v = 1.5 + 10.0 ** rng.uniform(-2, 2, L)[None, :, None] * rng.randn(N, L, d)
    w = rng.uniform(0.1, 3.0, d)
    first, second, cross = ref.segment_moments(v, w)
    f, s2, sx, F, A2, Ax = ref.moments_ld(v, w)
    b2, bx = 2 * (N * d + 9) * U * A2, 2 * (2 * N + d + 9) * U * Ax
    assert (np.abs(first.astype(LD) - f) <= 2 * N * U * F).all()
    assert (np.abs(second.astype(LD) - s2) <= b2).all() and (np.abs(cross.astype(LD) - sx) <= bx).all()
    cov = ref.unpack(ref.covariance_of(N, second, cross), L)
    bound = ref.unpack(((b2 + 4 * U * A2) + (bx + 4 * U * Ax) / N) / (N - 1), L)
    assert (np.abs(cov.astype(LD) - ref.covariance_ld(v, w)) <= bound).all()
    fast_w = ref.weights_pow2(d, 1)
    v26 = field_moments_ref.data26(N, L, d, 2)[0]
    assert all(same_bits(a, b) for a, b in zip(ref.segment_moments(v26, fast_w, exact_products=True), ref.segment_moments(v26, fast_w)))
    with pytest.raises(AssertionError):
        ref.segment_moments(v, fast_w, exact_products=True)
    with pytest.raises(AssertionError):
        ref.segment_moments(v26, w, exact_products=True)


def test_a_mean_far_above_the_standard_deviation_costs_no_digit():
    """N = 500 samples of L = 3 models with d = 6 components, unit variance around 1e8.  The largest error of an entry of the
    covariance against the two-pass long-double value, relative to sqrt(C_jj C_kk):
        shifted (Part 16)                                              1.6e-16
        unshifted, sum <y_j, y_k> - N <ybar_j, ybar_k> in float64      13.8
    The shifted sums keep all but the last few bits; the unshifted form has lost every digit (its error is of the order of the
    result and above: 1e16 u N against a variance of 1)."""
    N, L, d = 500, 3, 6
    rng = np.random.RandomState(11)
    v = 1e8 + rng.randn(N, L, d)
    w = rng.uniform(0.5, 2.0, d)
    want = ref.covariance_ld(v, w)
    scale = np.sqrt(np.outer(np.diag(want), np.diag(want))).astype(np.float64)
    _, second, cross = ref.segment_moments(v, w)
    shifted = np.abs((ref.unpack(ref.covariance_of(N, second, cross), L).astype(LD) - want).astype(np.float64)) / scale
    ybar = v.mean(axis=0)
    plain = (np.einsum("ijc,c,ikc->jk", v, w, v) - N * np.einsum("jc,c,kc->jk", ybar, w, ybar)) / (N - 1)
    unshifted = np.abs((plain.astype(LD) - want).astype(np.float64)) / scale
    print("relative error of the covariance at mean 1e8: shifted", shifted.max(), "unshifted", unshifted.max())
    assert shifted.max() <= 2 * (N * d + 2 * N + d + 30) * U * 4       # the bound above with sum |w a b| <= about 4 sqrt(C_jj C_kk) (N - 1)
    assert unshifted.max() > 1e4 * shifted.max()


# ---- the mix-in -------------------------------------------------------------------------------------------------------------------
def numpy_covariances(segs):
    """per output {group: (N, C^ [L, L])} from numpy alone, two passes"""
    weights = [np.ones(1), MASS]
    out = [{}, {}]
    for g, vals in segs:
        for n in range(2):
            y = vals[n]
            dm = y - y.mean(axis=0, keepdims=True)
            N = y.shape[0]
            out[n][g] = (N, np.einsum("ijc,c,ikc->jk", dm, weights[n], dm) / (N - 1) if N >= 2 else np.full((y.shape[1],) * 2, np.nan))
    return out


def numpy_errors(p, W, covs):
    var, c = np.zeros(2), 0
    for g in np.flatnonzero(SAMPLES > 0).tolist():
        ls, m = GROUPS[g], int(SAMPLES[g])
        for n in range(2):
            u = W[n, c:c + len(ls)]
            if u.any():
                var[n] += m * float(u @ (covs[n][g][1] if m >= 2 else p.get_covariance(n)[np.ix_(ls, ls)]) @ u)
        c += len(ls)
    return np.sqrt(var)


def test_solve_replays_the_call_sequence_and_keeps_the_covariances(stubbed):
    from bluest_amd.moments import MomentsMixin
    from bluest_amd.sap import BLUESTError
    bases = _bases()
    plain = toy(*bases[1:])
    hand_set(plain)
    want = plain.solve(K=3, eps=[0.2, 0.3])
    assert not stubbed["cov"]                                           # without the new mix-in nothing changes
    p = toy(*bases)
    for method in (p.sampled_errors, p.pooled_covariances):
        with pytest.raises(BLUESTError):
            method()                                                    # before a solve()
    W = hand_set(p)
    mus, errs, cost = p.solve(K=3, eps=[0.2, 0.3])
    assert p.calls == plain.calls and len(p.calls) == sum(-(-int(m) // 16) for m in SAMPLES)
    assert isinstance(mus[0], float) and same_bits(mus[0], want[0][0]) and same_bits(mus[1], want[0][1])
    assert same_bits(errs, want[1]) and cost == want[2]
    segs, _ = segments_drawn(p)
    chosen = np.flatnonzero(SAMPLES > 0).tolist()
    assert len(stubbed["cov"]) == 2 and not stubbed["err"]              # one flush: ONE call per output
    for n, (values, w) in enumerate(stubbed["cov"]):
        assert [v.shape for v in values] == [(int(SAMPLES[g]), len(GROUPS[g]), (1, D)[n]) for g in chosen]
        assert np.array_equal(w, (np.ones(1), MASS)[n]) and all(np.array_equal(v, s[1][n]) for v, s in zip(values, segs))
    want_covs = numpy_covariances(segs)
    for n in range(2):
        assert sorted(p.field_sample_covariances[n]) == chosen
        for g in chosen:
            N, C = p.field_sample_covariances[n][g]
            assert N == int(SAMPLES[g]) and C.shape == (len(GROUPS[g]),) * 2 and same_bits(C, C.T)
            assert np.allclose(C, want_covs[n][g][1], rtol=1e-10, atol=0, equal_nan=True) and np.isnan(C).all() == (N < 2)
    assert np.allclose(p.sampled_errors(), numpy_errors(p, W, want_covs), rtol=1e-10, atol=0)
    assert np.allclose(p.sampled_errors(source="model"), errs, rtol=1e-15, atol=0)
    with pytest.raises(ValueError):
        p.sampled_errors(source="pilot")
    # pooled: MomentsMixin's own formula on the per-group covariances, entry for entry
    covs = p.field_sample_covariances
    stand_in = types.SimpleNamespace(_sampled=lambda: {g: (covs[0][g][0], np.stack([covs[0][g][1], covs[1][g][1]])) for g in chosen},
                                     MOSAP_output=p.MOSAP_output, n_outputs=2, M=p.M, get_covariance=p.get_covariance)
    want_Cs, want_dof = MomentsMixin.pooled_covariances(stand_in)
    Cs, dof = p.pooled_covariances()
    assert all(same_bits(a, b) for a, b in zip(Cs, want_Cs)) and all(same_bits(a, b) for a, b in zip(dof, want_dof))
    assert dof[0][0, 1] == 8 and dof[0][1, 1] == 8 + 39 + 4 and dof[0][0, 0] == 8          # group 4 = [0, 2] was drawn once
    assert all(np.isfinite(C).all() and np.allclose(C, C.T) for C in Cs)
    q = toy(*bases[1:])                                                 # the pooled matrices go on as C
    q.__init__(p.M, C=Cs, costs=np.array([4.0, 2.0, 1.0]), n_outputs=2, verbose=False, sample_batch_size=16)
    assert all(np.array_equal(q.get_covariance(n), Cs[n]) for n in range(2))
    # a variance test's repeats are not looked at, and leave the covariances of the solve alone
    before = [dict(m) for m in covs]
    p.variance_test(eps=[0.2, 0.3], K=3, N=2)
    assert len(stubbed["cov"]) == 2 and all(a[g][1] is b[g][1] for a, b in zip(p.field_sample_covariances, before) for g in chosen)


def test_the_hook_chains_in_front_of_the_field_errors(stubbed):
    """FieldCovariancesMixin first: both mix-ins see every flush, each ONE call per output, and the two error bars are the same
    quantity, u' C^ u against the variance of z = u' y, to rounding"""
    from bluest_amd.field_errors import FieldErrorsMixin
    both, alone = toy(*_bases(errors=True)), toy(*_bases())
    hand_set(both)
    hand_set(alone)
    both.solve(K=3, eps=[0.2, 0.3])
    assert len(stubbed["cov"]) == 2 and len(stubbed["err"]) == 2
    alone.solve(K=3, eps=[0.2, 0.3])
    chosen = np.flatnonzero(SAMPLES > 0).tolist()
    for n in range(2):
        assert sorted(both.field_sample_moments[n]) == chosen
        assert all(same_bits(both.field_sample_covariances[n][g][1], alone.field_sample_covariances[n][g][1]) for g in chosen)
    assert np.allclose(both.sampled_errors(), FieldErrorsMixin.sampled_errors(both), rtol=1e-10, atol=0)
    maps, unsampled = both.sampled_error_fields()
    assert maps[1].shape == (D,)
    behind = toy(*((_bases(errors=True)[1], _bases()[0]) + _bases()[1:]))                  # the wrong order: the segments never arrive
    hand_set(behind)
    behind.solve(K=3, eps=[0.2, 0.3])
    assert behind.field_sample_covariances == [{}, {}] and len(stubbed["cov"]) == 4


def test_what_is_refused(stubbed):
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.sap import BLUESTError
    FieldCovariancesMixin, _, SamplingMixin, BLUEProblem = _bases()
    kw = dict(C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False)
    q = type("Q", (FieldCovariancesMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem), {})(2, **kw)
    for refused in (q.reorder_graph_nodes, q.reorder_all_graph_nodes):
        with pytest.raises(BLUESTError):
            refused()
    from bluest_amd.pilot import PilotMixin
    with pytest.raises(BLUESTError):                                    # sample files stay refused (PilotMixin is where they would be read)
        type("S", (FieldCovariancesMixin, FieldOutputsMixin, SamplingMixin, PilotMixin, BLUEProblem), {})(2, samplefile="samples.npz", **kw)

    class Inner(FieldCovariancesMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem):
        def get_models_inner_products(self):
            return [lambda a, b: float(np.dot(a, b))]

    class NoSampling(FieldCovariancesMixin, FieldOutputsMixin, BLUEProblem):
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
        assert p.field_sample_covariances is None
        p.field_sample_covariances, p.MOSAP_output = [{}], {}
        for method in (p.sampled_errors, p.pooled_covariances):
            with pytest.raises(BLUESTError):
                method()
    assert not stubbed["cov"]
    assert not hasattr(FieldCovariancesMixin, "variance_test") and not hasattr(FieldCovariancesMixin, "complexity_test")    # inherited untouched
    # MomentsMixin keeps refusing fields
    from bluest_amd.moments import MomentsMixin
    m = type("M", (MomentsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem), {})(2, **kw)
    with pytest.raises(BLUESTError):
        m.sampled_errors()

"""
Host tests of bluest_amd.moments: the build and the binding of bluest_group_moments, the argument checks of group_moments, the numpy
restatement of Part 13 (tests/moments_ref.py) against long-double sums, the covariance formula against np.cov, and MomentsMixin
with the restatements standing in for both kernels over the tests/golden/estimator_case_*.npz fixtures: the sampler is called as
the reference called it, sample_moments holds every sampled group, pooled_covariances is the direct pooling, the refusals are in
place.  The allocation and the weights are set by hand here (tests/test_gpu_moments.py runs the real ones).
"""
import ctypes

import numpy as np
import pytest

import gsums_ref
import moments_ref
from test_estimator_host import FakeComm, hand_set

CASES = gsums_ref.case_names()
U = gsums_ref.U


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.moments import MomentsMixin
    return MomentsMixin, SamplingMixin, BLUEProblem


@pytest.fixture
def stubbed(monkeypatch):
    """group_sums and group_moments -> their restatements; the segments of every group_moments call are kept"""
    from bluest_amd import estimator, moments
    seen = []

    def fake_moments(values, slab_bytes=None):
        seen.append(values)
        return moments_ref.group_moments(values)
    monkeypatch.setattr(estimator, "group_sums", lambda values, weights=None, repeat_of=None, R=None, slab_bytes=None:
                        gsums_ref.group_sums(values, weights, repeat_of, R))
    monkeypatch.setattr(moments, "group_moments", fake_moments)
    return seen


def general(n_out, N, L, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models"""
    rng = np.random.RandomState(seed)
    return 1.5 + 10.0 ** rng.uniform(-3, 3, L) * rng.randn(n_out, N, L)


# ---- the build and the binding ----------------------------------------------------------------------------------------------------
def test_the_unit_is_built_and_the_symbol_bound():
    from bluest_amd import _lib, build
    assert "moments.hip" in build.SOURCES
    build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bluest_group_moments")
    assert len(_lib.SIGNATURES["bluest_group_moments"]) == 8
    assert _lib.lib().bluest_group_moments.argtypes == _lib.SIGNATURES["bluest_group_moments"]


def test_group_moments_checks_its_segments():
    import torch
    from bluest_amd import moments
    with pytest.raises(ValueError):
        moments.group_moments([])
    with pytest.raises(ValueError):
        moments.group_moments([np.ones((1, 4, 2)), np.ones((2, 4, 2))])
    with pytest.raises(ValueError):
        moments.group_moments([np.ones((4, 2))])
    with pytest.raises(ValueError):
        moments.group_moments([torch.ones(1, 4, 2, dtype=torch.float32)])
    with pytest.raises(ValueError):
        moments.group_covariances([])


def test_group_moments_has_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bluest_amd import _lib, moments
    with pytest.raises(_lib.BluestHipError):
        moments.group_moments([np.ones((1, 4, 2))])
    first, second = np.full((1, 2), -7.0), np.full((1, 3), -7.0)
    v = np.ones((1, 4, 2))
    ptrs = (ctypes.c_void_p * 1)(_lib.ptr(v))
    counts, sizes = np.array([4], dtype=np.int64), np.array([2], dtype=np.int32)
    rc = _lib.lib().bluest_group_moments(1, 1, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                         _lib.ptr(first), _lib.ptr(second), None)
    assert rc == 3 and (first == -7.0).all() and (second == -7.0).all()             # BLUEST_ERR_NOGPU, nothing written
    assert _lib.lib().bluest_group_moments(0, 1, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                           _lib.ptr(first), _lib.ptr(second), None) == 1  # the arguments are checked first


# ---- the restatement --------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("shape", [(2, 1, 3), (2, 2, 3), (1, 17, 5), (2, 129, 4), (1, 300, 7), (1, 40, 33)])
def test_the_restatement_is_inside_the_rounding_bound(shape):
    v = general(*shape, seed=sum(shape))
    N = shape[1]
    first, second = moments_ref.segment_moments(v)
    s1, s2, a1, a2 = moments_ref.moments_ld(v)
    assert (np.abs(first.astype(gsums_ref.LD) - s1) <= 2 * N * U * a1).all()
    assert (np.abs(second.astype(gsums_ref.LD) - s2) <= 2 * N * U * a2).all()
    if N == 1:
        assert (first == 0).all() and (second == 0).all() and not np.signbit(first).any() and not np.signbit(second).any()


def test_exact_products_take_the_fast_path_to_the_same_bits():
    """on data whose products are exact, q + a * b has the bits of the fma: the restatement's two forms agree, and the order of
    the additions still shows (the plain long-double sum differs in some entries)"""
    v = moments_ref.data26(2, 150, 5, 3)
    assert moments_ref.few_bits(moments_ref.shifted(v)) and not moments_ref.few_bits(moments_ref.shifted(general(1, 9, 3, 1)))
    slow, fast = moments_ref.segment_moments(v), moments_ref.segment_moments(v, exact_products=True)
    assert gsums_ref.same_bits(slow[0], fast[0]) and gsums_ref.same_bits(slow[1], fast[1])
    exact = moments_ref.moments_ld(v)[1].astype(np.float64)
    assert (fast[1] != exact).any()
    with pytest.raises(AssertionError):
        moments_ref.segment_moments(general(1, 9, 3, 1), exact_products=True)


def test_the_covariance_formula_agrees_with_numpy():
    from bluest_amd import moments
    rng = np.random.RandomState(11)
    A = rng.randn(4, 4) + 2 * np.eye(4) + 1.0                           # every entry of A A' is of order one
    v = 3.0 + rng.randn(2, 200, 4) @ A.T
    first, second = moments_ref.segment_moments(v)
    C = moments.covariance_of(200, first, moments_ref.unpack(second, 4))
    for n in range(2):
        assert np.allclose(C[n], np.cov(v[n].T), rtol=1e-12, atol=0)
    assert np.isnan(moments.covariance_of(1, first, moments_ref.unpack(second, 4))).all()
    assert np.isnan(moments.covariance_of(0, first, moments_ref.unpack(second, 4))).all()


def test_the_packed_triangles_are_unpacked_per_segment():
    from bluest_amd import moments
    sizes, counts = np.array([3, 1, 3, 5, 1], dtype=np.int32), np.array([4, 0, 2, 9, 1], dtype=np.int64)
    tri = sizes * (sizes + 1) // 2
    rng = np.random.RandomState(2)
    first, second = rng.randn(2, sizes.sum()), rng.randn(2, tri.sum())
    c = p = 0
    for (N, f, m), L, P, n in zip(moments._unpacked(counts, sizes, first, second), sizes, tri, counts):
        assert N == n and np.array_equal(f, first[:, c:c + L]) and np.array_equal(m, moments_ref.unpack(second[:, p:p + P], L))
        c, p = c + L, p + P


# ---- the mix-in -------------------------------------------------------------------------------------------------------------------
def direct_pooling(g, segs, model_C):
    """numpy alone: per output the pooled covariance and its degrees of freedom"""
    M, n_out = int(g["M"]), int(g["n_outputs"])
    Cs, dofs = [], []
    for n in range(n_out):
        acc, dof = np.zeros((M, M)), np.zeros((M, M))
        for ls, v in segs:
            if v.shape[1] >= 2:
                acc[np.ix_(ls, ls)] += (v.shape[1] - 1) * np.cov(v[n].T).reshape(len(ls), len(ls))
                dof[np.ix_(ls, ls)] += v.shape[1] - 1
        C = model_C[n].copy()
        C[dof > 0] = acc[dof > 0] / dof[dof > 0]
        Cs.append(C)
        dofs.append(dof)
    return Cs, dofs


@pytest.mark.parametrize("name", CASES)
def test_solve_replays_the_call_sequence_and_keeps_the_moments(name, stubbed):
    from bluest_amd.sap import BLUESTError
    g = gsums_ref.case(name)
    n_calls, n_out = int(g["solve_calls"]), int(g["n_outputs"])
    MomentsMixin, SamplingMixin, BLUEProblem = _classes()
    plain = gsums_ref.replay_class(g, SamplingMixin, BLUEProblem)()
    hand_set(plain, g)
    want = plain.solve(K=int(g["K"]), eps=float(g["eps"]))
    p = gsums_ref.replay_class(g, MomentsMixin, SamplingMixin, BLUEProblem)()
    with pytest.raises(BLUESTError):
        p.sampled_errors()                                              # before a solve()
    with pytest.raises(BLUESTError):
        p.pooled_covariances()
    W = hand_set(p, g)
    mus, errs, cost = p.solve(K=int(g["K"]), eps=float(g["eps"]))
    assert p.calls == g["call_list"][:n_calls] and len(stubbed) == 1   # the reference's calls; ONE group_moments call
    assert gsums_ref.same_bits(mus, want[0]) and gsums_ref.same_bits(errs, want[1]) and cost == want[2]
    segs = gsums_ref.segments_of(g, 0, n_calls)
    chosen = np.flatnonzero(g["samples"] > 0)
    assert sorted(p.sample_moments) == chosen.tolist() and len(segs) == len(chosen)
    for gi, (ls, v) in zip(chosen.tolist(), segs):
        N, C = p.sample_moments[gi]
        assert g["groups"][gi] == ls and N == int(g["samples"][gi]) == v.shape[1] and C.shape == (n_out, len(ls), len(ls))
        if N >= 2:
            scale = np.sqrt(np.einsum("njj->nj", C))
            want_C = np.array([np.cov(v[n].T).reshape(len(ls), len(ls)) for n in range(n_out)])
            assert (np.abs(C - want_C) <= 1e-10 * scale[:, :, None] * scale[:, None, :]).all()
        else:
            assert np.isnan(C).all()
    # the error bars: the formula on the same draws, from numpy alone
    for source in ("samples", "model"):
        var, c = np.zeros(n_out), 0
        for gi, (ls, v) in zip(chosen.tolist(), segs):
            for n in range(n_out):
                w = W[n, c:c + len(ls)]
                C = np.cov(v[n].T).reshape(len(ls), len(ls)) if source == "samples" and v.shape[1] >= 2 else g["C"][n][np.ix_(ls, ls)]
                var[n] += v.shape[1] * (w @ C @ w)
            c += len(ls)
        assert np.allclose(p.sampled_errors(source=source), np.sqrt(var), rtol=1e-10, atol=0)
    with pytest.raises(ValueError):
        p.sampled_errors(source="pilot")
    Cs, dofs = p.pooled_covariances()
    want_Cs, want_dofs = direct_pooling(g, segs, g["C"])
    for n in range(n_out):
        assert np.array_equal(dofs[n], want_dofs[n]) and (dofs[n] > 0).any() and (dofs[n] == 0).any()
        assert np.allclose(Cs[n], want_Cs[n], rtol=1e-10, atol=0, equal_nan=True)
        assert np.array_equal(Cs[n][dofs[n] == 0], g["C"][n][dofs[n] == 0], equal_nan=True)
    # a variance test's repeats are not looked at, and leave the moments of the solve alone
    before = dict(p.sample_moments)
    p.start, p.calls = n_calls, []
    p.variance_test(eps=float(g["eps"]), K=int(g["K"]), N=2)
    assert len(stubbed) == 1 and sorted(p.sample_moments) == sorted(before)


def test_the_moments_are_taken_on_rank_0_after_the_gather(stubbed):
    MomentsMixin, SamplingMixin, BLUEProblem = _classes()

    class P(MomentsMixin, SamplingMixin, BLUEProblem):
        def sampler(self, ls, N=1):
            return [100.0 * self.mpiRank + np.arange(N)] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[s * (1 + l) for s, l in zip(samples, ls)]]

    board, size, results = {}, 3, {}
    samples, groups = np.array([0, 7, 4]), [[0], [0, 1], [1]]
    for rank in (2, 1, 0):                                              # rank 0 last: it finds the others' shares gathered
        p = P(2, C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False, sample_batch_size=3, comm=FakeComm(rank, size, board))
        out = {"budget": None, "eps": [0.1], "samples": samples, "flattened_groups": groups, "variances": np.ones(1), "cost": 1.0}
        p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (np.ones((1, 3)), np.ones(1)))
        p._collecting = {}                                              # what solve() does around the draw (the ranks of this
        p._sample_estimators(1)                                         # board run one after the other: no broadcast to wait for)
        results[rank] = p._collecting
    assert len(stubbed) == 1 and [v.shape for v in stubbed[0]] == [(1, 7, 2), (1, 4, 1)]        # the kernel runs on rank 0 alone
    col = stubbed[0][0][0, :, 0]
    assert col.tolist() == [0, 1, 2, 100, 101, 200, 201]               # 7 = 3 + 2 + 2, in rank order
    assert sorted(results[0]) == [1, 2] and results[0][1][0] == 7 and results[1] == {} and results[2] == {}
    assert np.allclose(results[0][1][1][0], np.cov(np.stack([col, 2 * col])), rtol=1e-12)


def test_what_is_refused(stubbed):
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.sap import BLUESTError
    MomentsMixin, SamplingMixin, BLUEProblem = _classes()
    kw = dict(C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False)
    q = type("Q", (MomentsMixin, SamplingMixin, BLUEProblem), {})(2, **kw)
    for refused in (q.reorder_graph_nodes, q.reorder_all_graph_nodes):
        with pytest.raises(BLUESTError):
            refused()

    class Inner(MomentsMixin, SamplingMixin, BLUEProblem):
        def get_models_inner_products(self):
            return [lambda a, b: float(np.dot(a, b))]

    class Field(MomentsMixin, FieldOutputsMixin, BLUEProblem):
        pass

    for cls, parent in ((Inner, BLUEProblem), (Field, FieldOutputsMixin)):
        p = cls(2, **kw)
        taken = []
        orig = parent.solve
        try:
            parent.solve = lambda self, **a: taken.append(sorted(a)) or "parent"
            assert p.solve(eps=0.1) == "parent" and len(taken) == 1 and "optimization_solver_params" in taken[0]
        finally:
            parent.solve = orig
        p.sample_moments, p.MOSAP_output = {}, {}
        with pytest.raises(BLUESTError):
            p.sampled_errors()
        with pytest.raises(BLUESTError):
            p.pooled_covariances()
    assert not stubbed
    assert not hasattr(MomentsMixin, "variance_test") and not hasattr(MomentsMixin, "complexity_test")     # inherited untouched
    assert Inner.variance_test is SamplingMixin.variance_test and Inner.complexity_test is SamplingMixin.complexity_test


# ---- the formula is unbiased -----------------------------------------------------------------------------------------------------
def test_the_sampled_variance_is_unbiased_under_a_wrong_model_covariance(monkeypatch):
    """Three models, the groups {0,1,2}, {1,2}, {2} drawn 12, 40 and 150 times from C_true, while the weights come from a model
    covariance with smaller variances and stronger correlations.  Over R = 400 independent solves the mean of sampled_errors()^2 must
    lie within 5 of its own standard errors of the estimator's true variance sum_g m_g w' C_true w -- which the model's promise
    (source="model") misses by far more.  np.cov stands in for the kernel: this is about the formula."""
    from bluest_amd import estimator, moments
    MomentsMixin, SamplingMixin, BLUEProblem = _classes()
    C_model = np.array([[1.0, 0.6, 0.3], [0.6, 1.2, 0.5], [0.3, 0.5, 0.9]])
    C_true = np.array([[2.5, 1.0, 0.4], [1.0, 2.0, 0.6], [0.4, 0.6, 2.2]])
    groups, m = [[0, 1, 2], [1, 2], [2]], np.array([12, 40, 150])
    Phi = np.zeros((3, 3))
    for ls, mg in zip(groups, m):
        Phi[np.ix_(ls, ls)] += mg * np.linalg.inv(C_model[np.ix_(ls, ls)])
    v = np.linalg.inv(Phi)[0]
    W = np.concatenate([np.linalg.inv(C_model[np.ix_(ls, ls)]) @ v[ls] for ls in groups])[None, :]
    promised = float(np.linalg.inv(Phi)[0, 0])
    true_var = sum(mg * w @ C_true[np.ix_(ls, ls)] @ w for ls, mg, w in zip(groups, m, np.split(W[0], [3, 5])))

    def numpy_moments(values, slab_bytes=None):
        out = []
        for y in values:
            d = y - y[:, :1, :]
            out.append((y.shape[1], d.sum(axis=1), np.einsum("nij,nik->njk", d, d)))
        return out
    monkeypatch.setattr(moments, "group_moments", numpy_moments)
    monkeypatch.setattr(estimator, "group_sums", lambda values, weights=None, repeat_of=None, R=None, slab_bytes=None:
                        ([y.sum(axis=1) for y in values], (weights * np.concatenate([y.sum(axis=1) for y in values], axis=1)).sum(axis=1)[None, :]))

    class Toy(MomentsMixin, SamplingMixin, BLUEProblem):
        def sampler(self, ls, N=1):
            z = self.rng.multivariate_normal(np.zeros(len(ls)), C_true[np.ix_(ls, ls)], size=N)
            return [z[:, i] for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            return [[2.0 + s for s in samples]]

    p = Toy(3, C=C_model, costs=np.array([4.0, 2.0, 1.0]), verbose=False, sample_batch_size=64)
    p.rng = np.random.RandomState(2024)
    out = {"budget": None, "eps": [0.1], "samples": m, "flattened_groups": groups, "variances": np.array([promised]), "cost": 1.0}
    p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (W, np.array([promised])))
    R, est, mus = 400, [], []
    for _ in range(R):
        mu, errs, _ = p.solve(eps=0.1)
        mus.append(mu[0])
        est.append(p.sampled_errors()[0] ** 2)
    est = np.array(est)
    se = est.std(ddof=1) / np.sqrt(R)
    print("true variance", true_var, "mean of the sampled variances", est.mean(), "+-", se, "promised by the model", promised,
          "variance of the", R, "estimates", np.var(mus, ddof=1))
    assert abs(est.mean() - true_var) <= 5 * se
    assert abs(promised - true_var) > 20 * se                           # the model's promise is not the truth here
    assert np.isclose(p.sampled_errors(source="model")[0] ** 2, promised, rtol=1e-12)
    assert abs(np.var(mus, ddof=1) / true_var - 1) < 5 * np.sqrt(2.0 / (R - 1))     # and the truth is what the estimates show

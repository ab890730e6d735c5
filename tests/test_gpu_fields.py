"""
GPU tests of bluest_amd.fields.FieldOutputsMixin end to end: the reference's weighted-inner-product pilot case
(tests/golden/pilot_case_inner.npz) through the real kernel, and a seeded problem with one number and one field of five components
per model against the host path on the same draws -- the same class without the mix-in and with hand-written inner products,
which BLUEProblem samples one Python call at a time; and the reference's own solve() and variance_test() on such a problem
(tests/golden/fields_estimator.npz, tools/gen_golden_fields.py) replayed with its recorded allocation.

The bound on an estimate is that of tests/test_gpu_estimator.py, per component: mu[c] = sum over the columns of w_col s_col[c];
two parties that add the same N_col values in different orders differ in s_col[c] by at most 2 N_col u sum|y|, and their weights,
from different factorisations of the same Phi (condition number kappa, blocks kappa_g), by 16 M u (kappa + max kappa_g) relatively.
"""
import numpy as np
import pytest

import fields_ref
import pilot_ref
from fields_ref import same_bits
from pilot_ref import scatter, within

pytestmark = pytest.mark.gpu

U = fields_ref.U
LD = np.longdouble
M, D = 4, 5
MASS = np.array([0.5, 1.0, 2.0, 1.0, 0.25])                            # the weights of the field's inner product
AMP = np.array([1.0, -0.5, 2.0, 0.1, 3.0])                              # component c of the field is AMP[c] * model(1, ...) + c


def test_the_reference_inner_product_case_through_the_kernel():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.pilot import PilotMixin
    g = pilot_ref.case("inner")
    w, N = g["vec_weights"], int(g["N"])

    class P(pilot_ref.replay_class(g, FieldOutputsMixin, PilotMixin, BLUEProblem)):
        def output_weights(self): return [w.copy() for n in range(self.n_outputs)]

    p = P(skip_projection=True)
    assert p.calls == g["call_list"]
    Y = np.stack(g["blocks"], axis=1)
    bounds = [fields_ref.cov_bound(Y[n], w, N) for n in range(Y.shape[0])]
    within(np.array(p.get_covariances()), g["cov"], scatter(g, np.stack([b[0] for b in bounds])))
    within(np.array(p.get_mlmc_variances()), g["dV"], scatter(g, np.stack([b[1] for b in bounds])))
    assert np.array_equal(p.get_costs(), g["costs"]) and [list(sg) for sg in p.SG] == pilot_ref.unpadded(g["SG"])


def model(n, l, z, e):
    """the toy model of tests/test_gpu_estimator.py"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def exact_covariance(n):
    a, d = 1 + 0.3 * n, 0.1 * n
    b, c = 0.9 ** np.arange(M), 0.1 * (np.arange(M) + 1)
    return a * a * np.outer(b, b) + 2 * d * d + np.diag(a * a * c * c)


COV = [exact_covariance(0), float(np.dot(AMP * MASS, AMP)) * exact_covariance(1)]
EPS = [0.25, 0.25 * float(np.sqrt(COV[1][0, 0]))]


def problem(with_mixin, seed=7):
    """one number and one field per model, a batch of one sample per call (what the host path draws); evaluate records what it
    returns; `on_device` makes it return CUDA tensors"""
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.fields import FieldOutputsMixin

    class Toy(*((FieldOutputsMixin,) if with_mixin else ()), SamplingMixin, BLUEProblem):
        on_device = False

        def sampler(self, ls, N=1):
            self.calls.append((list(ls), N))
            d = self.rng.randn(N, 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            Ps = [[float(model(0, l, *samples[i])[0]) for i, l in enumerate(ls)],
                  [AMP * float(model(1, l, *samples[i])[0]) + np.arange(D) for i, l in enumerate(ls)]]
            self.drawn.append((list(ls), Ps))
            if self.on_device:
                import torch
                return [[torch.tensor(v, dtype=torch.float64, device="cuda") for v in row] for row in Ps]
            return Ps

    if with_mixin:
        Toy.output_weights = lambda self: [None, MASS]
    else:
        Toy.get_models_inner_products = lambda self: [lambda a, b: a * b, lambda a, b: float(np.dot(a * MASS, b))]
    p = Toy(M, C=[c.copy() for c in COV], costs=2.0 ** -np.arange(M), n_outputs=2, verbose=False, sample_batch_size=1)
    p.rng, p.drawn, p.calls = np.random.RandomState(seed), [], []
    return p


def estimate_bounds(p, drawn):
    """per output the bound [d_n] on the difference of two parties' estimates from the values `drawn` of ONE estimator (the
    calls of every chosen group in list order), with weights made by numpy alone"""
    from test_gpu_estimator import numpy_weights
    out = p.MOSAP_output
    groups = [[int(i) for i in gr] for gr in out["flattened_groups"]]
    samples = np.asarray(out["samples"])
    W, K = numpy_weights({"M": M, "n_outputs": 2, "C": COV, "groups": groups, "samples": samples})
    chosen = [(gr, int(m)) for gr, m in zip(groups, samples) if m > 0]
    assert len(drawn) == sum(m for _, m in chosen)
    bounds, k = [np.zeros(1, dtype=LD), np.zeros(D, dtype=LD)], 0
    spread = [np.zeros(1, dtype=LD), np.zeros(D, dtype=LD)]
    col = 0
    for gr, m in chosen:
        assert all(ls == gr for ls, _ in drawn[k:k + m])
        for n in range(2):
            V = np.array([[np.atleast_1d(Ps[n][j]) for j in range(len(gr))] for _, Ps in drawn[k:k + m]]).astype(LD)   # [m, L, d]
            wcol = np.abs(W[n][col:col + len(gr)]).astype(LD)[:, None]
            bounds[n] += (wcol * 2 * m * U * np.abs(V).sum(axis=0)).sum(axis=0)
            spread[n] += (wcol * np.abs(V.sum(axis=0))).sum(axis=0)
        k += m
        col += len(gr)
    return [(b + 16 * M * U * K[n] * s).astype(np.float64) for n, (b, s) in enumerate(zip(bounds, spread))]


@pytest.fixture(scope="module")
def solved():
    """solve() on both paths, once"""
    f, h = problem(True), problem(False)
    return f, f.solve(K=3, eps=EPS), h, h.solve(K=3, eps=EPS)


def test_solve_agrees_with_the_host_path_on_the_same_draws(solved):
    f, (mus, errs, cost), h, (mus_h, errs_h, cost_h) = solved
    assert f.get_models_inner_products()[1](AMP, MASS) == h.get_models_inner_products()[1](AMP, MASS)
    assert np.array_equal(f.MOSAP_output["samples"], h.MOSAP_output["samples"])          # the allocations are identical
    assert f.calls == h.calls and len(f.calls) == int(np.sum(f.MOSAP_output["samples"]))   # and so are the sampler calls
    assert isinstance(mus[0], float) and isinstance(mus[1], np.ndarray) and mus[1].shape == (D,)
    bounds = estimate_bounds(h, h.drawn)
    print("estimates", mus, "host path", mus_h, "|diff| / bound", [np.abs(np.asarray(a) - np.asarray(b)) / bd for a, b, bd in zip(mus, mus_h, bounds)])
    for a, b, bd in zip(mus, mus_h, bounds):
        assert (np.abs(np.asarray(a) - np.asarray(b)) <= bd).all()
    assert np.allclose(errs, errs_h, rtol=1e-11) and cost == cost_h
    assert abs(mus[0] - 1.5) < 6 * errs[0]                              # (and it estimates what it should: E = 1.5, 1.6 AMP + c)


def test_device_resident_values_give_the_bits_of_host_arrays(solved):
    f, (mus, errs, cost) = solved[:2]
    q = problem(True)
    q.on_device = True
    mus_dev, errs_dev, _ = q.solve(K=3, eps=EPS)
    assert q.calls == f.calls and same_bits(mus_dev[0], mus[0]) and same_bits(mus_dev[1], mus[1]) and same_bits(errs_dev, errs)


def test_solve_mc_agrees_with_the_host_path():
    f, h = problem(True, seed=8), problem(False, seed=8)
    (mu, errs, cost), (mu_h, errs_h, cost_h) = f.solve_mc(eps=EPS), h.solve_mc(eps=EPS)
    N = len(h.drawn)
    assert f.calls == h.calls == [([0], 1)] * N and cost == cost_h == N * 1.0 and np.array_equal(errs, errs_h)
    for n in range(2):
        V = np.array([np.atleast_1d(Ps[n][0]) for _, Ps in h.drawn])   # [N, d]
        bound = 2 * N * U * np.abs(V).sum(axis=0) / N + U * np.abs(np.atleast_1d(mu_h[n]))
        assert (np.abs(np.atleast_1d(mu[n]) - np.atleast_1d(mu_h[n])) <= bound).all()
        assert same_bits(np.atleast_1d(mu[n]), fields_ref.segment_sums(V[:, None, :])[0] / N)
    assert isinstance(mu[0], float) and mu[1].shape == (D,)


def test_variance_test_agrees_with_the_host_path():
    """err^2 = s2 / N - <s1, s1> / N^2.  With every estimate off by at most b (per component) and A = the largest |estimate|,
    each of the two terms moves by at most 2 <A, b>, and its N (+ d for the inner product) additions by (N + d + 2) u <A, A> on
    either side: err^2 moves by at most 4 <A, b> + 4 (N + d + 2) u <A, A> =: delta, and err by at most delta / err."""
    N = 6
    f, h = problem(True, seed=9), problem(False, seed=9)
    estimates = []
    plain = h.solve
    h.solve = lambda **kw: (lambda r: (estimates.append(r[0]), r)[1])(plain(**kw))
    (err_ex, err), (err_ex_h, err_h) = f.variance_test(eps=EPS, K=3, N=N), h.variance_test(eps=EPS, K=3, N=N)
    assert f.calls == h.calls and np.array_equal(err_ex, err_ex_h) and len(estimates) == N
    per = len(h.drawn) // N
    inners = h.get_models_inner_products()
    for n, w in enumerate((np.ones(1), MASS)):
        b = np.max([estimate_bounds(h, h.drawn[r * per:(r + 1) * per])[n] for r in range(N)], axis=0)
        A = np.max([np.abs(np.atleast_1d(m[n])) for m in estimates], axis=0)
        delta = 4 * float(np.dot(A * w, b)) + 4 * (N + len(w) + 2) * U * float(np.dot(A * w, A))
        print("output", n, "err", err[n], "host path", err_h[n], "allowed", delta / err_h[n])
        assert abs(err[n] - err_h[n]) <= delta / err_h[n]
    assert ((err > 0.2 * err_ex) & (err < 3 * err_ex)).all()            # six estimates: the right size, no more
    assert inners[0](2.0, 3.0) == 6.0


# ---- the reference's own run on a field-valued output (tests/golden/fields_estimator.npz, tools/gen_golden_fields.py) -------------
def recorded():
    """the fixture with its calls split up: call_list [(ls, 1)], blocks[call] = ([L] numbers, [L, d] field values)"""
    from conftest import golden
    g = golden("fields_estimator.npz")
    d = len(g["mass"])
    calls, blocks, off = [], [], 0
    for row in g["calls"]:
        L = int(row[1])
        calls.append(([int(l) for l in row[2:2 + L]], int(row[0])))
        blocks.append((g["values"][off:off + L], g["values"][off + L:off + L + L * d].reshape(L, d)))
        off += L + L * d
    assert off == g["values"].size
    g["call_list"], g["blocks"] = calls, blocks
    return g


def replay(g, start):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.fields import FieldOutputsMixin

    class Replay(FieldOutputsMixin, SamplingMixin, BLUEProblem):
        def output_weights(self): return [None, g["mass"]]

        def sampler(self, ls, N=1):
            self.calls.append(([int(l) for l in ls], int(N)))
            return [start + len(self.calls) - 1] * len(ls)

        def evaluate(self, ls, samples, N=1):
            numbers, field = g["blocks"][samples[0]]
            self.drawn.append((list(ls), [[float(v) for v in numbers], [v.copy() for v in field]]))
            return self.drawn[-1][1]

    p = Replay(M, C=[c.copy() for c in g["C"]], costs=g["costs"].copy(), n_outputs=2, verbose=False, sample_batch_size=1)
    p.calls, p.drawn = [], []
    return p


def test_the_reference_field_estimator_is_replayed(monkeypatch):
    import gsums_ref
    from bluest_amd import mosap
    g = recorded()
    assert np.array_equal(g["mass"], MASS) and np.allclose(g["C"], COV, rtol=1e-15)
    monkeypatch.setattr(mosap.MOSAP, "solve", gsums_ref.fixed_allocation(g["samples"]))
    n_calls, N = int(g["solve_calls"]), int(g["vt_N"])
    p = replay(g, 0)
    mus, errs, cost = p.solve(K=int(g["K"]), eps=list(g["eps"]))
    assert p.calls == g["call_list"][:n_calls]
    assert [[int(i) for i in gr] for gr in p.MOSAP_output["flattened_groups"]] == [[int(i) for i in row if i >= 0] for row in g["flattened_groups"]]
    bounds = estimate_bounds(p, p.drawn)
    print("mus", mus, "reference", g["mu0"], g["mu1"], "|diff| / bound", abs(mus[0] - g["mu0"]) / bounds[0], np.abs(mus[1] - g["mu1"]) / bounds[1])
    assert abs(mus[0] - float(g["mu0"])) <= bounds[0][0] and (np.abs(mus[1] - g["mu1"]) <= bounds[1]).all()
    assert np.allclose(errs, g["errs"], rtol=1e-11) and abs(cost / float(g["cost"]) - 1) < 1e-11
    # variance_test: the bound of test_variance_test_agrees_with_the_host_path, with A from the estimates of this run widened by
    # their bounds (the reference's single estimates are not recorded)
    q = replay(g, n_calls)
    plain, record = q._sample_estimators, []
    q._sample_estimators = lambda n_rep: (lambda r: (record.append(r), r)[1])(plain(n_rep))
    err_ex, err = q.variance_test(N=N, K=int(g["K"]), eps=list(g["eps"]))
    assert q.calls == g["call_list"][n_calls:] and np.allclose(err_ex, g["vt_err_ex"], rtol=1e-11)
    estimates = record[0]                                               # per output [N, d_n]
    for n, w in enumerate((np.ones(1), MASS)):
        b = np.max([estimate_bounds(q, q.drawn[r * n_calls:(r + 1) * n_calls])[n] for r in range(N)], axis=0)
        A = np.max(np.abs(estimates[n]), axis=0) + b
        delta = 4 * float(np.dot(A * w, b)) + 4 * (N + len(w) + 2) * U * float(np.dot(A * w, A))
        print("output", n, "err", err[n], "reference", g["vt_err"][n], "allowed", delta / g["vt_err"][n])
        assert abs(err[n] - g["vt_err"][n]) <= delta / g["vt_err"][n]

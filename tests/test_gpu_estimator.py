"""
GPU tests of bluest_amd.estimator.SamplingMixin: the tests/golden/estimator_case_*.npz fixtures (one solve() and one
variance_test(N=50) of the reference on a hand-picked allocation, tools/gen_golden_estimator.py) replayed with MOSAP.solve set to
the recorded allocation; device-resident model values; solve_mc through the batched sampling; and one run with the real
optimiser, nothing replaced.

The bound on an estimate.  mu_o = sum_c w_c s_c over the columns c of the sampled groups, s_c a sum of N_c values y, w = C_g^-1 v_g
with v = row 0 of pinv(Phi_o).  Two parties that add the same values in different orders differ in s_c by at most
2 N_c u sum|y| (u = 2^-53), hence in mu by sum_c |w_c| 2 N_c u sum|y|.  Their weights come from different factorisations of the
same Phi_o (condition number kappa) built from differently rounded C_g^-1 (condition numbers kappa_g): a backward-stable solve of
an M x M system is off by at most about 8 M u kappa relatively, on either side, and so is each block; with
K_o = kappa(Phi_o) + max_g kappa(C_g) the weights contribute 16 M u K_o sum_c |w_c s_c|.  `mu_bound` is the sum of the two, from
numpy-made weights, never from the code under test.
"""
import numpy as np
import pytest

import gsums_ref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

TOL = 1e-11
U = gsums_ref.U
LD = np.longdouble
CASES = gsums_ref.case_names()


def _problem_class(g):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    return gsums_ref.replay_class(g, SamplingMixin, BLUEProblem)


def _solve_args(g):
    kw = dict(K=int(g["K"]), eps=float(g["eps"]))
    if "multi_groups" in g:
        kw["multi_groups"] = [[list(gr) for gr in mg] for mg in g["multi_groups"]]
    return kw


@pytest.fixture
def fixed(monkeypatch):
    """MOSAP.solve -> the fixture's allocation, as the generator did to the reference"""
    from bluest_amd import mosap

    def use(g):
        monkeypatch.setattr(mosap.MOSAP, "solve", gsums_ref.fixed_allocation(g["samples"]))
    return use


def numpy_weights(g):
    """per output: the weights over the columns of the sampled groups in list order, from numpy alone, and K_o of the bound"""
    M, n_out = int(g["M"]), int(g["n_outputs"])
    chosen = [(gr, int(m)) for gr, m in zip(g["groups"], g["samples"]) if m > 0]
    W, K = [], []
    for n in range(n_out):
        C = g["C"][n]
        mine = (lambda gr: True) if "multi_groups" not in g else (lambda gr, s={tuple(x) for x in g["multi_groups"][n]}: tuple(gr) in s)
        Phi, kappa_g = np.zeros((M, M)), 1.0
        for gr, m in chosen:
            if mine(gr):
                Phi[np.ix_(gr, gr)] += m * np.linalg.inv(C[np.ix_(gr, gr)])
                kappa_g = max(kappa_g, np.linalg.cond(C[np.ix_(gr, gr)]))
        idx = np.flatnonzero(np.diag(Phi) != 0)
        assert idx[0] == 0
        v = np.zeros(M)
        v[idx] = np.linalg.pinv(Phi[np.ix_(idx, idx)])[0]
        W.append(np.concatenate([np.linalg.inv(C[np.ix_(gr, gr)]) @ v[gr] if mine(gr) else np.zeros(len(gr)) for gr, _ in chosen]))
        K.append(np.linalg.cond(Phi[np.ix_(idx, idx)]) + kappa_g)
    return np.array(W), np.array(K)


def mu_bound(g, segs, W, K):
    """(numpy's estimates in long double, the bound of the module docstring) for the values `segs` of one estimator"""
    M = int(g["M"])
    sums = np.concatenate([v.astype(LD).sum(axis=1) for _, v in segs], axis=1)
    absolute = np.concatenate([np.abs(v).astype(LD).sum(axis=1) for _, v in segs], axis=1)
    counts = np.concatenate([[v.shape[1]] * v.shape[2] for _, v in segs])
    mu = (W.astype(LD) * sums).sum(axis=1)
    bound = (np.abs(W) * 2 * counts * U * absolute).sum(axis=1) + 16 * M * U * K * (np.abs(W) * np.abs(sums)).sum(axis=1)
    return mu.astype(np.float64), bound.astype(np.float64)


@pytest.mark.parametrize("name", CASES)
def test_solve_replays_the_reference(name, fixed):
    g = gsums_ref.case(name)
    fixed(g)
    n_calls, n_out = int(g["solve_calls"]), int(g["n_outputs"])
    p = _problem_class(g)()
    mus, errs, cost = p.solve(**_solve_args(g))
    assert [list(gr) for gr in p.MOSAP_output["flattened_groups"]] == g["groups"]
    assert p.calls == g["call_list"][:n_calls]
    segs = gsums_ref.segments_of(g, 0, n_calls)
    W, K = numpy_weights(g)
    mu_np, bound = mu_bound(g, segs, W, K)
    print(name, "mus", mus, "reference", g["mus"], "|diff| / bound", np.abs(np.array(mus) - g["mus"]) / bound, "kappa", K)
    assert (np.abs(np.array(mus) - g["mus"]) <= bound).all()
    assert (np.abs(np.array(mus) - mu_np) <= bound).all()
    assert (np.abs(errs / g["errs"] - 1) < TOL).all() and abs(cost / float(g["cost"]) - 1) < TOL
    # the estimator the host path forms from the same sums
    where = {tuple(ls): gsums_ref.segment_sums(v) for ls, v in segs}
    sums = [[list(where[tuple(gr)][n]) if tuple(gr) in where else [0] * len(gr) for gr in g["groups"]] for n in range(n_out)]
    mus_host, Vs_host = p.MOSAP.compute_BLUE_estimators(sums, g["samples"])
    assert (np.abs(np.array(mus) - np.array(mus_host)) <= bound).all() and (np.abs(np.sqrt(Vs_host) / errs - 1) < TOL).all()
    # device-resident values: evaluate returns CUDA tensors, the same bits come out
    q = _problem_class(g)()
    q.on_device = True
    mus_dev, errs_dev, _ = q.solve(**_solve_args(g))
    assert q.calls == p.calls and same_bits(mus_dev, mus) and same_bits(errs_dev, errs)


@pytest.mark.parametrize("name", CASES)
def test_variance_test_replays_the_reference(name, fixed):
    g = gsums_ref.case(name)
    fixed(g)
    n_calls, N = int(g["solve_calls"]), int(g["vt_N"])
    p = _problem_class(g)(start=n_calls)
    err_ex, err = p.variance_test(N=N, **_solve_args(g))
    assert p.calls == g["call_list"][n_calls:]
    assert (np.abs(err_ex / g["vt_err_ex"] - 1) < TOL).all()
    W, K = numpy_weights(g)
    bound = np.max([mu_bound(g, gsums_ref.segments_of(g, (r + 1) * n_calls, n_calls), W, K)[1] for r in range(N)], axis=0)
    # err^2 = s2 / N - s1^2 / N^2 is the difference of two numbers of size mean^2.  An error delta in every estimate moves each
    # of them by 2 |mean| delta at most, and adding N terms moves each by N u mean^2 more, on either side of the comparison: err^2
    # moves by (4 |mean| delta + 4 N u mean^2), and err, relatively, by half of that over err^2:
    # (2 delta / |mean| + 2 N u) * mean^2 / err^2 -- the relative bound on an estimate times the cancellation factor.
    factor = g["mus"] ** 2 / g["vt_err"] ** 2
    allowed = (2 * bound / np.abs(g["mus"]) + 2 * N * U) * factor
    print(name, "err", err, "reference", g["vt_err"], "relative difference", np.abs(err / g["vt_err"] - 1), "allowed", allowed)
    assert (np.abs(err / g["vt_err"] - 1) <= allowed).all()


def model(n, l, z, e):
    """the toy model of the fixtures (tools/gen_golden_estimator.py)"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def exact_covariance(M, n):
    a, d = 1 + 0.3 * n, 0.1 * n
    b, c = 0.9 ** np.arange(M), 0.1 * (np.arange(M) + 1)
    return a * a * np.outer(b, b) + 2 * d * d + np.diag(a * a * c * c)


def toy_problem(M, n_out, batch, seed, *more_bases):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin

    class Toy(SamplingMixin, *more_bases, BLUEProblem):
        def sampler(self, ls, N=1):
            d = self.rng.randn(N, 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            Ps = [[model(n, l, *samples[i]) for i, l in enumerate(ls)] for n in range(n_out)]
            self.drawn.append((list(ls), np.array(Ps)))
            return Ps

    p = Toy(M, C=[exact_covariance(M, n) for n in range(n_out)], costs=2.0 ** -np.arange(M), n_outputs=n_out, verbose=False,
            sample_batch_size=batch)
    p.rng, p.drawn = np.random.RandomState(seed), []
    return p


def test_solve_mc_through_the_mixin_equals_the_plain_sum():
    p = toy_problem(3, 2, 8, 41)
    mu, errs, cost = p.solve_mc(eps=0.25)
    N = int(np.ceil(max(exact_covariance(3, n)[0, 0] / 0.25 ** 2 for n in range(2))))
    assert [b.shape[2] for _, b in p.drawn] == [8] * (N // 8) + ([N % 8] if N % 8 else []) and cost == N * 1.0
    values = np.concatenate([b for _, b in p.drawn], axis=2).transpose(0, 2, 1)       # [n_out, N, 1]
    assert same_bits(np.array(mu), gsums_ref.segment_sums(values)[:, 0] / N)
    assert (np.abs(np.array(mu) - values.sum(axis=1)[:, 0] / N) <= 2 * N * U * np.abs(values).sum(axis=1)[:, 0] / N + U * np.abs(mu)).all()


def test_end_to_end_with_the_real_optimiser():
    """nothing replaced: M = 5, K = 3, two outputs, eps = 0.1 (sigma_0 = 1.005 and 1.31).  C is exact, so the variance the
    allocation promises is the estimator's: the standard deviation of 50 estimates has a relative standard error of about
    1 / sqrt(2 * 49) = 0.1, and [0.6, 1.5] is four of them either way.  Halving eps four times multiplies the cost by 4 each time
    as long as rounding to whole samples and the one-sample floor of model 0 do not matter: a rate of 2."""
    p = toy_problem(5, 2, 64, 42)
    err_ex, err = p.variance_test(eps=0.1, K=3, N=50)
    print("variance test: promised", err_ex, "observed", err, "ratio", err / err_ex)
    assert ((err >= 0.6 * err_ex) & (err <= 1.5 * err_ex)).all()
    tot_cost, rate = p.complexity_test([0.1, 0.05, 0.025, 0.0125], K=3)
    print("complexity test: costs", tot_cost, "rate", rate)
    assert 1.7 <= rate <= 2.3

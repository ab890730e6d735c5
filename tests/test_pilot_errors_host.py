"""CPU tests of bluest_amd.pilot_errors: the build and the binding of bluest_pilot_moments4, the host arithmetic of the standard
errors against the two-pass long-double restatement and the Wishart value, and PilotErrorsMixin with the restatements of
tests/pilot_ref.py and tests/pilot4_ref.py standing in for both kernels: PilotMixin's sampler calls and bits without a tolerance,
the growth rule of the adaptive pilot with one, three ranks, and the refusals."""
import ctypes
import math
import os
import threading

import numpy as np
import pytest

import pilot4_ref
import pilot_ref
from conftest import GOLDEN

SCALAR_CASES = [c for c in pilot_ref.case_names() if c != "inner"]


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.pilot import PilotMixin
    from bluest_amd.pilot_errors import PilotErrorsMixin
    return PilotErrorsMixin, PilotMixin, BLUEProblem


@pytest.fixture
def stubbed(monkeypatch):
    """pilot_statistics and pilot_fourth_moments -> their restatements; the values of every call are kept"""
    from bluest_amd import pilot, pilot_errors
    seen = {"stats": [], "fourth": []}

    def stats(values, differences=True):
        seen["stats"].append(values)
        return pilot_ref.pilot_statistics(values, differences)

    def fourth(values, differences=True, shift=None, slab_bytes=None):
        seen["fourth"].append(values)
        return pilot4_ref.pilot_fourth_moments(values, differences, shift)
    monkeypatch.setattr(pilot, "pilot_statistics", stats)
    monkeypatch.setattr(pilot_errors, "pilot_fourth_moments", fourth)
    return seen


# ---- the build and the binding ----------------------------------------------------------------------------------------------------
def test_the_unit_is_built_and_the_symbol_bound():
    from bluest_amd import _lib, build
    assert "pilot4.hip" in build.SOURCES
    build.build()
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bluest_pilot_moments4")
    assert len(_lib.SIGNATURES["bluest_pilot_moments4"]) == 11
    assert _lib.lib().bluest_pilot_moments4.argtypes == _lib.SIGNATURES["bluest_pilot_moments4"]
    assert _lib.lib().bluest_abi_version() == 1


def test_the_wrapper_checks_its_arguments():
    import torch
    from bluest_amd import pilot_errors
    for bad in (np.ones((4, 2)), torch.ones(1, 4, 2, dtype=torch.float32)):
        with pytest.raises(ValueError):
            pilot_errors.pilot_fourth_moments(bad)
    with pytest.raises(ValueError):
        pilot_errors.pilot_fourth_moments(np.ones((2, 4, 3)), shift=np.ones(3))


# ---- the host arithmetic ------------------------------------------------------------------------------------------------------------
def test_the_float64_emulation_of_the_chunked_order_stays_inside_the_bound():
    """the order of the additions of Part 14 in float64 without fma (one more rounding per term, still at most 8): inside
    (N + 16) u sum|term|, and in fact far inside it (a tenth of it here), as a bound that counts every rounding at its worst is"""
    worst = 0.0
    for N, L in ((300, 5), (129, 33)):
        Y = np.random.default_rng(3).normal(1e3, 1.0, size=(2, N, L))
        got, ref, bound = pilot4_ref.chunked_f64(Y), pilot4_ref.sums_ld(Y), pilot4_ref.bounds(Y)
        for g, r, b in zip(got, ref, bound):
            err = np.abs(g.astype(pilot4_ref.LD) - r).astype(np.float64)
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
            assert (err <= b).all()
    print("largest error / bound:", worst)


def test_the_shifted_one_pass_form_agrees_with_two_passes():
    from bluest_amd import pilot_errors
    rng = np.random.default_rng(1)
    C = np.array([[1.0, 0.9, 0.3], [0.9, 1.0, 0.5], [0.3, 0.5, 2.0]])
    Y = rng.multivariate_normal([5.0, -3.0, 1e3], C, size=2000)[None]
    _, first, s11, s21, s22, tpow = pilot4_ref.pilot_fourth_moments(Y)
    se_c, se_d = pilot_errors.pilot_standard_errors(2000, first, s11, s21, s22, tpow)
    ref_c, ref_d = pilot4_ref.standard_errors(Y)
    iu = np.triu_indices(3, 1)
    assert np.abs(se_c / ref_c - 1).max() <= 1e-12 and np.abs(se_d[0][iu] / ref_d[0][iu] - 1).max() <= 1e-12
    assert np.isnan(se_d[0][np.tril_indices(3)]).all()
    only_c, none = pilot_errors.pilot_standard_errors(2000, first, s11, s21, s22)
    assert none is None and np.array_equal(only_c, se_c)
    for N in (0, 1):
        a, b = pilot_errors.pilot_standard_errors(N, first, s11, s21, s22, tpow)
        assert np.isnan(a).all() and np.isnan(b).all()


def test_gaussian_samples_give_the_wishart_value():
    """N = 4000 samples of a known 3 x 3 covariance: SE(C^_ij) within 10 % of sqrt((C_ii C_jj + C_ij^2) / (N - 1)) (the estimate of
    a fourth moment from 4000 samples is itself good to a few per cent), and SE(dV^) within 10 % of dV sqrt(2 / (N - 1))"""
    from bluest_amd import pilot_errors
    N = 4000
    C = np.array([[1.0, 0.9, 0.3], [0.9, 1.0, 0.5], [0.3, 0.5, 2.0]])
    Y = np.random.default_rng(0).multivariate_normal([5.0, -3.0, 1e3], C, size=N)[None]
    _, first, s11, s21, s22, tpow = pilot4_ref.pilot_fourth_moments(Y)
    se_c, se_d = pilot_errors.pilot_standard_errors(N, first, s11, s21, s22, tpow)
    var = np.diag(C)
    wishart = np.sqrt((np.outer(var, var) + C ** 2) / (N - 1))
    assert np.abs(se_c[0] / wishart - 1).max() <= 0.10, np.abs(se_c[0] / wishart - 1).max()
    iu = np.triu_indices(3, 1)
    dV = (var[:, None] + var[None, :] - 2 * C)[iu]
    assert np.abs(se_d[0][iu] / (dV * np.sqrt(2.0 / (N - 1))) - 1).max() <= 0.10


# ---- the mix-in without a tolerance: PilotMixin, and the errors of what it estimated --------------------------------------------------
@pytest.mark.parametrize("name", SCALAR_CASES)
def test_without_a_tolerance_the_mixin_is_pilotmixin_plus_one_call(name, stubbed):
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()
    g = pilot_ref.case(name)
    N, L, M, n_out = int(g["N"]), len(g["ls"]), int(g["M"]), int(g["n_outputs"])
    p = pilot_ref.replay_class(g, PilotErrorsMixin, PilotMixin, BLUEProblem)(skip_projection=True)
    assert p.calls == g["call_list"]                                   # the reference's sampler calls, in its order
    assert [v.shape for v in stubbed["stats"]] == [(n_out, N, L)] and [v.shape for v in stubbed["fourth"]] == [(n_out, N, L)]
    assert stubbed["fourth"][0] is stubbed["stats"][0]                  # the same gathered values
    values = stubbed["stats"][0]
    q = pilot_ref.replay_class(g, PilotMixin, BLUEProblem)(skip_projection=True)
    assert len(stubbed["stats"]) == 2 and len(stubbed["fourth"]) == 1
    for a, b in ((p.get_covariances(), q.get_covariances()), (p.get_mlmc_variances(), q.get_mlmc_variances())):
        assert np.array_equal(np.array(a).view(np.int64), np.array(b).view(np.int64))
    assert np.array_equal(p.get_costs(), q.get_costs()) and p.SG == q.SG
    assert p.pilot_report == {"samples": N, "rounds": 1, "ratio": None, "converged": True}
    # the errors: the restatement's, exactly where an entry was estimated
    ref_c, ref_d = pilot4_ref.standard_errors(values)
    ls = g["ls"]
    err_c, err_d = np.array(p.get_covariance_errors()), np.array(p.get_mlmc_variance_errors())
    assert err_c.shape == err_d.shape == (n_out, M, M)
    estimated = np.isnan(g["C_given"])
    pairs = ~np.isfinite(g["dV_given"]) & np.triu(np.ones((M, M), dtype=bool), 1)
    outside = np.ones(M, dtype=bool)
    outside[ls] = False
    pairs[:, outside, :] = pairs[:, :, outside] = False                 # only the sampled models have a difference to estimate
    assert np.array_equal(~np.isnan(err_c), estimated) and np.array_equal(~np.isnan(err_d), pairs)
    assert np.array_equal(err_c, err_c.transpose(0, 2, 1), equal_nan=True)
    want_c, want_d = np.full((n_out, M, M), np.nan), np.full((n_out, M, M), np.nan)
    want_c[np.ix_(range(n_out), ls, ls)], want_d[np.ix_(range(n_out), ls, ls)] = ref_c, ref_d
    for got, want, mask in ((err_c, want_c, estimated), (err_d, want_d, pairs)):
        assert mask.any() and np.abs(got[mask] / want[mask] - 1).max() <= 1e-12, np.abs(got[mask] / want[mask] - 1).max()
    assert np.array_equal(p.get_covariance_error(n_out - 1), err_c[n_out - 1], equal_nan=True)
    assert np.array_equal(p.get_mlmc_variance_error(n_out - 1), err_d[n_out - 1], equal_nan=True)


def test_an_entry_the_rho_rule_zeroed_keeps_its_error(stubbed):
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()
    table = np.array([[1.0, -1.0, 1.0, -1.0], [1.0, 1.0, -1.0, -1.0]])

    class P(PilotErrorsMixin, PilotMixin, BLUEProblem):
        drawn = 0

        def sampler(self, ls, N=1):
            self.drawn += 1
            return [self.drawn - 1] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[float(table[l, samples[i]]) for i, l in enumerate(ls)]]

    p = P(2, costs=[2.0, 1.0], covariance_estimation_samples=4, remove_uncorrelated=False, verbose=False)
    assert np.array_equal(p.get_covariance(), np.eye(2))                # exactly uncorrelated: written as 0
    err = p.get_covariance_error()
    assert np.isfinite(err).all() and err[0, 1] > 0                     # mu22 = 1: the estimate 0 has a sampling error


# ---- the adaptive pilot ---------------------------------------------------------------------------------------------------------------
MIX = np.array([[1.0, 0.0, 0.0], [0.9, 0.3, 0.0], [0.5, 0.2, 0.6]])


def _seeded_class(*bases, heavy=False):

    class P(*bases):
        k = 0

        def sampler(self, ls, N=1):                                     # seeded by its call count: call k gives what call k gives
            self.k += 1
            rng = np.random.default_rng(self.k)
            z = rng.standard_t(5, size=3) if heavy else rng.standard_normal(3)
            return [z] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[float(2.0 + MIX[l] @ samples[i]) for i, l in enumerate(ls)]]
    return P


def _ratio(values, tol):
    """the largest SE / (tol x scale) over all entries of C (scale sqrt(C^_ii C^_jj)) and of dV (scale dV^), from two passes"""
    se_c, se_d = pilot4_ref.standard_errors(values)
    C_hat, dV_hat = pilot4_ref.estimates(values)
    var = np.diagonal(C_hat, axis1=1, axis2=2)
    iu = np.triu_indices(values.shape[2], 1)
    r = (se_c / (tol * np.sqrt(var[:, :, None] * var[:, None, :]))).max()
    return float(max(r, (se_d[:, iu[0], iu[1]] / (tol * dV_hat[:, iu[0], iu[1]])).max()))


def _rule(N, r, size, N_max):
    want = max(N + size, min(4 * N, int(math.ceil(1.1 * N * r * r))))
    return min(N_max, size * (want // size + int(want % size > 0)))


def _run_adaptive(stubbed, heavy, tol=0.1, N0=20, **kw):
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()
    del stubbed["stats"][:], stubbed["fourth"][:]
    p = _seeded_class(PilotErrorsMixin, PilotMixin, BLUEProblem, heavy=heavy)(
        3, costs=[4.0, 2.0, 1.0], covariance_estimation_samples=N0, covariance_estimation_tol=tol, sample_batch_size=1,
        verbose=False, **kw)
    return p, list(stubbed["stats"]), list(stubbed["fourth"])


def test_the_pilot_grows_by_the_rule_and_stops_at_the_first_pass(stubbed):
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()
    tol, N0 = 0.1, 20
    p, stats, fourth = _run_adaptive(stubbed, heavy=False, tol=tol, N0=N0)
    sizes = [v.shape[1] for v in stats]
    assert sizes == [v.shape[1] for v in fourth] and sizes[0] == N0 and len(sizes) >= 2
    ratios = [_ratio(v, tol) for v in stats]
    for N, r, after in zip(sizes, ratios, sizes[1:]):
        assert r > 1 and after == _rule(N, r, 1, 64 * N0), (N, r, after)
    assert ratios[-1] <= 1                                              # it stopped at the first round that passes
    for a, b in zip(stats, stats[1:]):                                  # every round recomputes on all the samples so far
        assert np.array_equal(a, b[:, :a.shape[1]])
    assert p.k == sizes[-1]
    assert p.pilot_report["samples"] == sizes[-1] and p.pilot_report["rounds"] == len(sizes) and p.pilot_report["converged"]
    assert abs(p.pilot_report["ratio"] / ratios[-1] - 1) <= 1e-9
    # the result is the one of a single pilot of that size
    q = _seeded_class(PilotMixin, BLUEProblem)(3, costs=[4.0, 2.0, 1.0], covariance_estimation_samples=sizes[-1], sample_batch_size=1,
                                               verbose=False)
    assert np.array_equal(stubbed["stats"][-1], stats[-1])
    for a, b in ((p.get_covariances(), q.get_covariances()), (p.get_mlmc_variances(), q.get_mlmc_variances())):
        assert np.array_equal(np.array(a).view(np.int64), np.array(b).view(np.int64))
    ref_c, ref_d = pilot4_ref.standard_errors(stats[-1])
    iu = np.triu_indices(3, 1)
    assert np.abs(p.get_covariance_error() / ref_c[0] - 1).max() <= 1e-12
    assert np.abs(p.get_mlmc_variance_error()[iu] / ref_d[0][iu] - 1).max() <= 1e-12


def test_heavy_tails_need_more_rounds(stubbed):
    light, _, _ = _run_adaptive(stubbed, heavy=False)
    heavy, _, _ = _run_adaptive(stubbed, heavy=True)
    assert light.pilot_report["converged"] and heavy.pilot_report["converged"]
    assert heavy.pilot_report["rounds"] > light.pilot_report["rounds"]
    assert heavy.pilot_report["samples"] > light.pilot_report["samples"]


def test_a_tiny_cap_ends_unconverged_with_a_warning(stubbed, capsys):
    p, stats, _ = _run_adaptive(stubbed, heavy=False, covariance_estimation_max_samples=30)
    assert [v.shape[1] for v in stats] == [20, 30]
    assert p.pilot_report["samples"] == 30 and p.pilot_report["converged"] is False and p.pilot_report["ratio"] > 1
    assert "covariance_estimation_tol" in capsys.readouterr().out
    assert np.isfinite(p.get_covariance_error()).all()


# ---- three ranks ---------------------------------------------------------------------------------------------------------------------
class ThreadComm(object):
    """rank `rank` of `size`, one thread each; gather and bcast meet at a barrier"""

    def __init__(self, rank, size, shared):
        self.rank, self.size, self.shared = rank, size, shared

    def Get_rank(self): return self.rank
    def Get_size(self): return self.size
    def barrier(self): self.shared["barrier"].wait()

    def gather(self, obj, root=0):
        self.shared["slots"][self.rank] = obj
        self.barrier()
        out = list(self.shared["slots"]) if self.rank == root else None
        self.barrier()
        return out

    def bcast(self, obj, root=0):
        if self.rank == root:
            self.shared["value"] = obj
        self.barrier()
        out = self.shared["value"]
        self.barrier()
        return out


def test_three_ranks_sample_their_shares_and_rank_0_runs_the_kernels(stubbed):
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()
    size = 3
    shared = {"barrier": threading.Barrier(size, timeout=60), "slots": [None] * size, "value": None}
    problems, failures = {}, []
    ranks_of_calls = []

    class P(PilotErrorsMixin, PilotMixin, BLUEProblem):
        def sampler(self, ls, N=1):
            self.draws.append(len(self.draws))
            rng = np.random.default_rng(1000 * self.mpiRank + self.draws[-1])
            return [rng.standard_normal(3)] * len(ls)

        def evaluate(self, ls, samples, N=1):
            out = [float(2.0 + MIX[l] @ samples[i]) for i, l in enumerate(ls)]
            self.mine.append(out)
            return [out]

        def _pilot_gathered(self, ls, values):
            ranks_of_calls.append(self.mpiRank)
            return super()._pilot_gathered(ls, values)

    def run(rank):
        try:
            p = P.__new__(P)
            p.draws, p.mine = [], []
            p.__init__(3, costs=[4.0, 2.0, 1.0], covariance_estimation_samples=20, covariance_estimation_tol=0.25,
                       sample_batch_size=1, verbose=False, comm=ThreadComm(rank, size, shared))
            problems[rank] = p
        except BaseException as e:                                      # a failed rank must not leave the others waiting
            failures.append((rank, e))
            shared["barrier"].abort()

    threads = [threading.Thread(target=run, args=(r,)) for r in range(size)]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not failures, failures
    sizes = [v.shape[1] for v in stubbed["stats"]]
    assert sizes[0] == 21 and len(sizes) >= 2 and all(n % size == 0 for n in sizes)     # 20 rounded up to the three ranks
    assert [v.shape[1] for v in stubbed["fourth"]] == sizes             # both kernels once per round: on rank 0 alone
    assert set(ranks_of_calls) == {0} and len(ranks_of_calls) == len(sizes)
    # round-major, then in rank order, each rank's samples in the order it drew them
    at, rows = {r: 0 for r in range(size)}, []
    for before, after in zip([0] + sizes, sizes):
        share = (after - before) // size
        for r in range(size):
            rows += problems[r].mine[at[r]:at[r] + share]
            at[r] += share
    assert np.array_equal(stubbed["stats"][-1][0], np.array(rows))
    assert all(len(problems[r].mine) == sizes[-1] // size for r in range(size))
    for r in (1, 2):                                                    # every rank ends with rank 0's results
        assert problems[r].pilot_report == problems[0].pilot_report and problems[0].pilot_report["samples"] == sizes[-1]
        assert np.array_equal(problems[r].get_covariance(), problems[0].get_covariance())
        assert np.array_equal(problems[r].get_covariance_error(), problems[0].get_covariance_error())
        assert np.array_equal(problems[r].get_mlmc_variance_error(), problems[0].get_mlmc_variance_error(), equal_nan=True)


# ---- where the sums do not come from bluest_pilot_stats --------------------------------------------------------------------------------
def test_python_inner_products_behave_as_pilotmixin_and_refuse_a_tolerance(stubbed):
    from bluest_amd.sap import BLUESTError
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()
    g = pilot_ref.case("inner")
    P = pilot_ref.replay_class(g, PilotErrorsMixin, PilotMixin, BLUEProblem)
    p = P(skip_projection=True)
    q = pilot_ref.replay_class(g, PilotMixin, BLUEProblem)(skip_projection=True)
    assert p.calls == g["call_list"] == q.calls and stubbed["stats"] == [] and stubbed["fourth"] == []
    assert np.array_equal(np.array(p.get_covariances()), np.array(q.get_covariances()), equal_nan=True)
    assert np.array_equal(np.array(p.get_mlmc_variances()), np.array(q.get_mlmc_variances()), equal_nan=True)
    for call in (p.get_covariance_errors, p.get_covariance_error, p.get_mlmc_variance_errors, p.get_mlmc_variance_error):
        with pytest.raises(BLUESTError, match="inner products"):
            call()
    with pytest.raises(BLUESTError, match="inner products"):
        P(skip_projection=True, covariance_estimation_tol=0.1)


def test_field_outputs_refuse_a_tolerance():
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.sap import BLUESTError
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()

    class P(PilotErrorsMixin, FieldOutputsMixin, PilotMixin, BLUEProblem):
        def sampler(self, ls, N=1): pytest.fail("refused before anything is drawn")

    with pytest.raises(BLUESTError, match="FieldOutputsMixin"):
        P(2, costs=[2.0, 1.0], covariance_estimation_tol=0.1, verbose=False)


def test_a_loaded_problem_has_no_errors_and_refuses_a_tolerance():
    from bluest_amd.sap import BLUESTError
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()

    class P(PilotErrorsMixin, PilotMixin, BLUEProblem):
        pass

    path = os.path.join(GOLDEN, "pilot_graph_matern.npz")
    p = P(7, datafile=path, verbose=False)
    assert p.pilot_report is None
    with pytest.raises(BLUESTError, match="no standard errors"):
        p.get_covariance_errors()
    with pytest.raises(BLUESTError, match="model-graph file"):
        P(7, datafile=path, covariance_estimation_tol=0.1, verbose=False)
    for name in ("reorder_graph_nodes", "reorder_all_graph_nodes"):
        with pytest.raises(BLUESTError):
            getattr(p, name)()


def test_nothing_unknown_means_nothing_has_an_error(stubbed):
    PilotErrorsMixin, PilotMixin, BLUEProblem = _classes()

    class P(PilotErrorsMixin, PilotMixin, BLUEProblem):
        def sampler(self, ls, N=1): pytest.fail("nothing is unknown: nothing to sample")

    C = np.array([[2.0, 0.5, np.inf], [0.5, 1.0, 0.25], [np.inf, 0.25, 1.5]])
    p = P(3, C=C, costs=[4.0, 2.0, 1.0], covariance_estimation_tol=0.1, verbose=False)
    assert np.isnan(p.get_covariance_error()).all() and np.isnan(p.get_mlmc_variance_error()).all()
    assert p.pilot_report == {"samples": 0, "rounds": 0, "ratio": None, "converged": True} and stubbed["fourth"] == []

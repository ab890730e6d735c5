"""CPU tests of bluest_amd.field_pilot_errors: the build and the binding of bluest_field_pilot_moments, the restatement of Part 17
(tests/field_pilot_ref.py) against the long-double two-pass values within its derived bound, the host arithmetic of the standard
errors against the scalar formula at d = 1 and the Gaussian closed forms, and FieldPilotErrorsMixin with the restatements standing
in for field_statistics and field_pilot_moments: the sampler calls and bits of FieldOutputsMixin, the growth of the adaptive pilot,
both caps, a mixed number / field problem, three ranks' shares, and every refusal."""
import ctypes
import os
from fractions import Fraction

import numpy as np
import pytest

import field_pilot_ref as ref
import fields_ref
import pilot4_ref
from conftest import GOLDEN
from field_pilot_ref import LD, U, same_bits

MASS = np.array([0.5, 1.0, 2.0, 1.0, 0.25])
AMP = np.array([1.0, -0.5, 2.0, 0.1, 3.0])
D = 5


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.field_pilot_errors import FieldPilotErrorsMixin
    from bluest_amd.fields import FieldOutputsMixin
    from bluest_amd.pilot import PilotMixin
    return FieldPilotErrorsMixin, FieldOutputsMixin, PilotMixin, BLUEProblem


@pytest.fixture
def stubbed(monkeypatch):
    """field_statistics and field_pilot_moments -> their restatements; the arguments of every call are kept"""
    from bluest_amd import field_pilot_errors, fields
    seen = {"stats": [], "moments": []}

    def stats(values, w, differences=True):
        seen["stats"].append((values, np.array(w)))
        return fields_ref.field_statistics(values, w, differences)

    def moments(values, w, centre=None, differences=True, **kw):
        seen["moments"].append((values, np.array(w), None if centre is None else np.array(centre)))
        return ref.field_pilot_moments(values, w, centre, differences)
    monkeypatch.setattr(fields, "field_statistics", stats)
    monkeypatch.setattr(field_pilot_errors, "field_pilot_moments", moments)
    return seen


# ---- the build and the binding ----------------------------------------------------------------------------------------------------
def test_the_unit_is_built_and_the_symbols_bound():
    from bluest_amd import _lib, build, field_pilot_errors
    assert "field_pilot.hip" in build.SOURCES
    build.build()
    for name, nargs in (("bluest_field_pilot_moments", 13), ("bluest_field_pilot_scratch", 2)):
        assert hasattr(ctypes.CDLL(_lib.LIB_PATH), name) and len(_lib.SIGNATURES[name]) == nargs
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    header = open(os.path.join(os.path.dirname(GOLDEN), os.pardir, "include", "bluest_hip.h")).read()
    assert "#define BLUEST_FIELD_STRIP         %d" % field_pilot_errors.BLUEST_FIELD_STRIP in header and ref.STRIP == 512
    before = ctypes.c_int64(0)
    assert _lib.lib().bluest_field_pilot_scratch(0, ctypes.byref(before)) == 0 and before.value == 256 << 20
    with field_pilot_errors.scratch_limit(12345):
        assert _lib.lib().bluest_field_pilot_scratch(0, ctypes.byref(before)) == 0 and before.value == 12345
    assert _lib.lib().bluest_field_pilot_scratch(0, ctypes.byref(before)) == 0 and before.value == 256 << 20


def test_the_wrapper_checks_its_arguments_and_has_no_cpu_path():
    import torch
    from bluest_amd import _lib, field_pilot_errors
    for bad in (np.ones((4, 2)), torch.ones(4, 2, 3, dtype=torch.float32)):
        with pytest.raises(ValueError):
            field_pilot_errors.field_pilot_moments(bad, np.ones(3), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        field_pilot_errors.field_pilot_moments(np.ones((4, 2, 3)), np.ones(2), np.zeros((2, 3)))
    with pytest.raises(ValueError):
        field_pilot_errors.field_pilot_moments(np.ones((4, 2, 3)), np.ones(3), np.zeros((3, 2)))
    if not torch.cuda.is_available():
        with pytest.raises(_lib.BluestHipError):
            field_pilot_errors.field_pilot_moments(np.ones((4, 2, 3)), np.ones(3), np.zeros((2, 3)))


# ---- the restatement --------------------------------------------------------------------------------------------------------------
def _field(N, L, d, seed, mean=1.5):
    rng = np.random.RandomState(seed)
    Y = mean + rng.randn(N, L, d) * (1.0 if mean > 1e3 else 10.0 ** rng.uniform(-1, 1, (L, 1)))
    if L > 1:
        Y[:, 1] = Y[:, 0] + 1e-3 * rng.randn(N, d)
    return Y, rng.uniform(0.1, 2.0, d)


def _check_against_long_double(Y, w):
    N, L, d = Y.shape
    centre = np.asarray(Y.astype(LD).sum(axis=0), dtype=np.float64) / N
    got = ref.pilot_moments(Y, w, centre)
    q, r, _, _ = ref.per_sample_ld(Y, w, centre)
    upper = np.triu(np.ones((L, L)), 1).astype(LD)
    worst = 0.0
    for sums, x, bound, mask in ((got[:3], q, ref.bounds(Y, w, centre)[0], 1), (got[3:], r, ref.bounds(Y, w, centre)[1], upper)):
        want = [a * mask for a in ref.shifted_ld(x)]
        for g, v, b in zip(sums, want, bound[:3]):
            err = np.abs(g.astype(LD) - v).astype(np.float64)
            assert (err <= b).all(), (err.max(), b.max())
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    se_c, se_d = _se()(N, got[1], got[2], got[4], got[5])
    ld_c, ld_d = ref.standard_errors_ld(Y, w, centre)
    iu = np.triu_indices(L, 1)
    assert (np.abs(se_c - ld_c) <= ref.bounds(Y, w, centre)[0][3]).all()
    assert (np.abs(se_d[iu] - ld_d[iu]) <= ref.bounds(Y, w, centre)[1][3][iu]).all()
    return got, centre, worst, float(np.abs(se_c / ld_c - 1).max())


def _se():
    from bluest_amd.field_pilot_errors import field_pilot_standard_errors
    return field_pilot_standard_errors


@pytest.mark.parametrize("N,L,d", [(40, 3, 9), (130, 2, 65), (300, 4, 1), (5, 3, 600)])
def test_the_restatement_stays_inside_its_bound(N, L, d):
    _, _, worst, rel = _check_against_long_double(*_field(N, L, d, seed=N + d))
    print("largest error / bound:", worst, "largest relative error of SE(C^):", rel)


def test_a_mean_far_above_the_spread_costs_no_digit():
    """mean 1e8 over unit variance: the centred differences are exact (Sterbenz), so the bound -- stated in the centred values --
    is as small as at mean 0, and the standard errors keep their digits"""
    Y, w = _field(200, 3, 9, seed=5, mean=1e8)
    _, _, worst, rel = _check_against_long_double(Y, w)
    print("largest error / bound:", worst, "largest relative error of SE(C^):", rel)
    assert rel <= 1e-12


def test_the_per_sample_values_add_up_to_the_covariance_sums():
    """sum_s q_s = qs1 + N qfirst is sumsc - <sumse, sumse> / N when the centre is sumse / N; the centre is that mean rounded, which
    adds N <a delta, a delta>_w with |delta| <= u"""
    for mean in (1.5, 1e8):
        Y, w = _field(200, 3, 9, seed=6, mean=mean)
        N = Y.shape[0]
        got, centre, _, _ = _check_against_long_double(Y, w)
        F = np.frompyfunc(Fraction, 1, 1)                               # exactly: at mean 1e8 the two terms agree to 16 digits
        Yf, wf = F(Y), F(w)
        se = Yf.sum(axis=0)
        want = np.array([[float(sum((wf * Yf[s, i] * Yf[s, j]).sum() for s in range(N)) - (wf * se[i] * se[j]).sum() / N)
                          for j in range(3)] for i in range(3)]).astype(LD)
        bound = ref.bounds(Y, w, centre)[0]
        allowed = bound[1] + N * bound[0] + N * U * U * np.einsum("ic,c,jc->ij", np.abs(centre), w, np.abs(centre)) + 4 * U * np.abs(got[0]) * N + U * np.abs(want).astype(np.float64)
        assert (np.abs(got[1].astype(LD) + N * got[0].astype(LD) - want).astype(np.float64) <= allowed).all()


# ---- the standard errors ------------------------------------------------------------------------------------------------------------
def test_at_one_component_the_error_is_the_scalar_one_up_to_its_second_order_terms():
    """d = 1, N = 4000 Gaussian samples: pilot_standard_errors keeps the O(1 / N) terms -- the variance of the centre, 1 / (N - 1) on
    the Gaussian variance, and the factor (N - 1) / N --; the first-order error differs from it by about 1 / N relatively (measured
    here: below), asserted within 2 / N"""
    from bluest_amd import pilot_errors
    N = 4000
    C = np.array([[1.0, 0.9, 0.3], [0.9, 1.0, 0.5], [0.3, 0.5, 2.0]])
    Y = np.random.default_rng(0).multivariate_normal([5.0, -3.0, 1e3], C, size=N)
    _, first, s11, s21, s22, tpow = pilot4_ref.pilot_fourth_moments(Y[None])
    want_c, want_d = pilot_errors.pilot_standard_errors(N, first, s11, s21, s22, tpow)
    centre = (Y.astype(LD).sum(axis=0) / N).astype(np.float64)[:, None]
    _, qs1, qs2, _, rs1, rs2 = ref.pilot_moments(Y[:, :, None], np.ones(1), centre)
    se_c, se_d = _se()(N, qs1, qs2, rs1, rs2)
    iu = np.triu_indices(3, 1)
    rel = max(np.abs(se_c / want_c[0] - 1).max(), np.abs(se_d[iu] / want_d[0][iu] - 1).max())
    print("largest relative difference x N:", rel * N)
    assert rel <= 2.0 / N
    assert np.isnan(se_d[np.tril_indices(3)]).all()


@pytest.mark.parametrize("d", [5, 64])
def test_gaussian_fields_give_the_closed_forms(d):
    """(N, L, d) = (4000, 4, d), independent components of covariance S, random weights:
    SE(C^_ij) -> sqrt(sum_c w_c^2 (S_ii S_jj + S_ij^2) / N) and SE(dV^_ij) -> sqrt(2 sum_c w_c^2 D_ij^2 / N), D = S_ii + S_jj - 2 S_ij.
    The long-double two-pass reference alone lies within 3.8 % (d = 5) and 2.5 % (d = 64) of them on these draws (printed below):
    the scatter of a second moment of products of Gaussians estimated from 4000 samples, over sixteen entries.  The margin is
    some three to four times that, for other seeds: 10 %.  The restatement agrees with the reference to rounding."""
    N, L = 4000, 4
    rng = np.random.default_rng(d)
    A = rng.standard_normal((L, L))
    S = A @ A.T / L + 0.5 * np.eye(L)
    Y = 3.0 + rng.multivariate_normal(np.zeros(L), S, size=(N, d)).transpose(0, 2, 1)
    w = rng.uniform(0.2, 2.0, d)
    centre = (Y.astype(LD).sum(axis=0) / N).astype(np.float64)
    _, qs1, qs2, _, rs1, rs2 = ref.pilot_moments(Y, w, centre)
    se_c, se_d = _se()(N, qs1, qs2, rs1, rs2)
    var = np.diag(S)
    form_c = np.sqrt((w ** 2).sum() * (np.outer(var, var) + S ** 2) / N)
    form_d = np.sqrt(2 * (w ** 2).sum() * (var[:, None] + var[None, :] - 2 * S) ** 2 / N)
    iu = np.triu_indices(L, 1)
    ld_c, ld_d = ref.standard_errors_ld(Y, w, centre)
    print("long double against the closed forms:", float(np.abs(ld_c / form_c - 1).max()), float(np.abs(ld_d[iu] / form_d[iu] - 1).max()))
    assert np.abs(se_c / ld_c - 1).max() <= 1e-10 and np.abs(se_d[iu] / ld_d[iu] - 1).max() <= 1e-10
    assert np.abs(se_c / form_c - 1).max() <= 0.10 and np.abs(se_d[iu] / form_d[iu] - 1).max() <= 0.10
    assert np.array_equal(se_c, se_c.T)


def test_fewer_than_two_samples_have_no_error():
    z = np.zeros((3, 3))
    for N in (0, 1):
        a, b = _se()(N, z, z, z, z)
        assert np.isnan(a).all() and np.isnan(b).all()
        a, b = _se()(N, z, z)
        assert np.isnan(a).all() and b is None
    a, b = _se()(2, z, z)
    assert not a.any() and b is None


# ---- the mix-in ---------------------------------------------------------------------------------------------------------------------
MIX = np.array([[1.0, 0.3, 0.0], [0.9, 0.0, 0.4], [0.5, -0.6, 0.7]])
M = 3


def _seeded_class(*bases, weights=(None, MASS), device=False):
    """one number and one field of five components per model; the draws are seeded by the call count: call k gives what call k
    gives, however the calls are spread over rounds"""

    class P(*bases):
        k = 0
        calls = None

        def output_weights(self): return list(weights)

        def sampler(self, ls, N=1):
            self.k += 1
            type(self).calls = (self.calls or []) + [(list(ls), N)]
            z = np.random.default_rng(self.k).standard_normal((N, 3))
            return [z] * len(ls)

        def evaluate(self, ls, samples, N=1):
            number = [2.0 + samples[i] @ MIX[l] for i, l in enumerate(ls)]                     # [N2]
            out = [number if w is None else [AMP[:len(w)] * (v[:, None] + 0.1 * v[:, None] ** 2) + np.arange(len(w)) for v in number]
                   for w in weights]
            if device:
                import torch
                out = [[torch.tensor(v, dtype=torch.float64, device="cuda") for v in row] for row in out]
            return out
    return P


def _make(*bases, N0=20, batch=4, **kw):
    cls = _seeded_class(*bases, **{k: kw.pop(k) for k in ("weights", "device") if k in kw})
    weights = cls.output_weights(None)
    return cls(M, costs=[4.0, 2.0, 1.0], n_outputs=len(weights), covariance_estimation_samples=N0, sample_batch_size=batch, verbose=False,
               skip_projection=True, **kw)


def _bits(a):
    return np.ascontiguousarray(np.array(a, dtype=np.float64)).view(np.int64)


def test_without_a_tolerance_the_mixin_is_fieldoutputsmixin_plus_one_call_per_output(stubbed):
    E, F, PM, B = _classes()
    p = _make(E, F, PM, B)
    stats, moments = list(stubbed["stats"]), list(stubbed["moments"])
    q = _make(F, PM, B)
    assert type(p).calls == type(q).calls == [([0, 1, 2], 4)] * 5       # the sampler calls of FieldOutputsMixin
    assert [v.shape for v, _ in stats] == [(20, 3, 1), (20, 3, 5)] == [v.shape for v, _, _ in moments]
    assert len(stubbed["stats"]) == 4 and len(stubbed["moments"]) == 2  # (q made two more statistics calls and no moments call)
    for (v, w), (v2, w2, centre), (v3, _) in zip(stats, moments, stubbed["stats"][2:]):
        assert v2 is v and np.array_equal(w, w2) and np.array_equal(v, v3)      # the same gathered values, not a copy
        assert same_bits(centre, fields_ref.field_statistics(v, w, False)[0] / 20)   # the centre from the sums already returned
    assert np.array_equal(_bits(p.get_covariances()), _bits(q.get_covariances()))
    assert np.array_equal(_bits(p.get_mlmc_variances()), _bits(q.get_mlmc_variances()))
    assert p.pilot_report == {"samples": 20, "rounds": 1, "ratio": None, "converged": True, "capped_by": None}
    iu = np.triu_indices(M, 1)
    for n, (v, w, centre) in enumerate(moments):
        ld_c, ld_d = ref.standard_errors_ld(v, w, centre)
        assert np.abs(p.get_covariance_error(n) / ld_c - 1).max() <= 1e-10
        assert np.abs(p.get_mlmc_variance_error(n)[iu] / ld_d[iu] - 1).max() <= 1e-10
        assert np.isnan(p.get_mlmc_variance_error(n)[np.tril_indices(M)]).all()
        assert np.array_equal(p.get_covariance_errors()[n], p.get_covariance_error(n))
        assert np.array_equal(p.get_mlmc_variance_errors()[n], p.get_mlmc_variance_error(n), equal_nan=True)
    # a number of a mixed problem is a field of one component: its errors are those of the scalar formula up to 1 / N
    from bluest_amd import pilot_errors
    _, first, s11, s21, s22, tpow = pilot4_ref.pilot_fourth_moments(np.ascontiguousarray(moments[0][0].transpose(2, 0, 1)))
    scalar_c, _ = pilot_errors.pilot_standard_errors(20, first, s11, s21, s22, tpow)
    assert np.abs(p.get_covariance_error(0) / scalar_c[0] - 1).max() <= 0.25


def test_given_entries_have_no_error(stubbed):
    E, F, PM, B = _classes()
    C = np.full((M, M), np.nan)
    C[0, 0], C[0, 2], C[2, 0] = 2.0, 0.3, 0.3
    dV = np.full((M, M), np.nan)
    dV[0, 1] = 0.7
    p = _make(E, F, PM, B, C=[C.copy(), C.copy()], mlmc_variances=[dV.copy(), dV.copy()])
    for n in range(2):
        e, f = p.get_covariance_error(n), p.get_mlmc_variance_error(n)
        given = ~np.isnan(C)
        assert np.isnan(e[given]).all() and np.isfinite(e[~given]).all()
        assert np.isnan(f[0, 1]) and np.isfinite(f[0, 2]) and np.isfinite(f[1, 2]) and np.isnan(f[np.tril_indices(M)]).all()
        assert p.get_covariance(n)[0, 2] == 0.3 and p.get_mlmc_variance(n)[0, 1] == 0.7


def _ratio(kept, weights, tol):
    """the largest SE / (tol x scale) over the entries of C (scale sqrt(C^_ii C^_jj)) and dV (scale dV^), in long double"""
    worst = 0.0
    for v, w in zip(kept, weights):
        centre = (v.astype(LD).sum(axis=0) / v.shape[0]).astype(np.float64)
        q, r, _, _ = ref.per_sample_ld(v, w, centre)
        se_c, se_d = ref.standard_errors_ld(v, w, centre)
        C_hat, dV_hat = q.mean(axis=0), r.mean(axis=0)
        var = np.diagonal(C_hat)
        iu = np.triu_indices(v.shape[1], 1)
        worst = max(worst, float((se_c / (tol * np.sqrt(np.outer(var, var)))).max()), float((se_d[iu] / (tol * dV_hat[iu])).max()))
    return worst


def test_the_pilot_grows_by_the_rule_and_ends_with_the_one_shot_result(stubbed):
    from bluest_amd.pilot_errors import next_pilot_size
    E, F, PM, B = _classes()
    tol, N0 = 0.15, 20
    p = _make(E, F, PM, B, N0=N0, covariance_estimation_tol=tol)
    stats, moments = list(stubbed["stats"]), list(stubbed["moments"])
    sizes = [v.shape[0] for v, _ in stats[0::2]]
    assert sizes == [v.shape[0] for v, _, _ in moments[1::2]] and sizes[0] == N0 and len(sizes) >= 2
    ws = [np.ones(1), MASS]
    ratios = [_ratio([stats[2 * k][0], stats[2 * k + 1][0]], ws, tol) for k in range(len(sizes))]
    for N, r, after in zip(sizes, ratios, sizes[1:]):
        assert r > 1 and after == next_pilot_size(N, r, 1, 64 * N0), (N, r, after)
    assert ratios[-1] <= 1                                              # it stopped at the first round that passes
    for a, b in zip(stats, stats[2:]):                                  # every round sums all the values so far, round-major
        assert np.array_equal(a[0], b[0][:a[0].shape[0]])
    drawn = sum(n for _, n in type(p).calls)
    assert drawn == sizes[-1]                                           # every round drew only what was missing
    assert p.pilot_report["samples"] == sizes[-1] and p.pilot_report["rounds"] == len(sizes) and p.pilot_report["converged"]
    assert p.pilot_report["capped_by"] is None and abs(p.pilot_report["ratio"] / ratios[-1] - 1) <= 1e-9
    q = _make(F, PM, B, N0=sizes[-1])                                   # FieldOutputsMixin alone on the same values
    for (a, _), (b, _) in zip(stubbed["stats"][-2:], stats[-2:]):
        assert np.array_equal(a, b)
    assert np.array_equal(_bits(p.get_covariances()), _bits(q.get_covariances()))
    assert np.array_equal(_bits(p.get_mlmc_variances()), _bits(q.get_mlmc_variances()))


def test_the_sample_cap_and_the_byte_cap_end_unconverged(stubbed, capsys):
    E, F, PM, B = _classes()
    p = _make(E, F, PM, B, covariance_estimation_tol=0.01, covariance_estimation_max_samples=30)
    assert [v.shape[0] for v, _ in stubbed["stats"][0::2]] == [20, 30]
    assert p.pilot_report["samples"] == 30 and p.pilot_report["converged"] is False and p.pilot_report["ratio"] > 1
    assert p.pilot_report["capped_by"] == "samples" and "covariance_estimation_max_samples" in capsys.readouterr().out
    assert np.isfinite(p.get_covariance_error(1)).all()
    del stubbed["stats"][:]
    per_sample = M * D * 8                                              # the kept values of the field, the largest output
    p = _make(E, F, PM, B, covariance_estimation_tol=0.01, covariance_estimation_max_bytes=25 * per_sample + 7)
    assert [v.shape[0] for v, _ in stubbed["stats"][0::2]] == [20, 25]
    assert p.pilot_report["samples"] == 25 and p.pilot_report["converged"] is False and p.pilot_report["capped_by"] == "bytes"
    assert "covariance_estimation_max_bytes" in capsys.readouterr().out
    del stubbed["stats"][:]
    p = _make(E, F, PM, B, covariance_estimation_tol=0.01, covariance_estimation_max_bytes=1)     # the first round is always drawn
    assert [v.shape[0] for v, _ in stubbed["stats"][0::2]] == [20] and p.pilot_report["capped_by"] == "bytes"


def test_a_change_of_residence_between_rounds_is_refused(stubbed):
    from bluest_amd.sap import BLUESTError
    E, F, PM, B = _classes()

    class Tensorish(np.ndarray):
        data_ptr = None                                                 # what the mix-in tells a tensor by

    cls = _seeded_class(E, F, PM, B)
    plain = cls._gathered

    def gathered(self, mine):
        out = plain(self, mine)
        return [v.view(Tensorish) for v in out] if self.k > 5 else out
    cls._gathered = gathered
    with pytest.raises(BLUESTError, match="device memory in this round"):
        cls(M, costs=[4.0, 2.0, 1.0], n_outputs=2, covariance_estimation_samples=20, covariance_estimation_tol=0.01, sample_batch_size=4,
            verbose=False, skip_projection=True)


def test_three_ranks_draw_their_shares_of_what_is_missing(stubbed):
    import threading
    from test_pilot_errors_host import ThreadComm
    E, F, PM, B = _classes()
    size, problems, failures = 3, {}, []
    shared = {"barrier": threading.Barrier(size, timeout=60), "slots": [None] * size, "value": None}

    def run(rank):
        try:
            cls = _seeded_class(E, F, PM, B)
            cls.k = 1000 * rank
            problems[rank] = cls(M, costs=[4.0, 2.0, 1.0], n_outputs=2, covariance_estimation_samples=20, sample_batch_size=4,
                                 covariance_estimation_tol=0.01, covariance_estimation_max_samples=40, verbose=False, skip_projection=True,
                                 comm=ThreadComm(rank, size, shared))
        except BaseException as e:                                      # a failed rank must not leave the others waiting
            failures.append((rank, e))
            shared["barrier"].abort()
    threads = [threading.Thread(target=run, args=(r,)) for r in range(size)]
    for t in threads: t.start()
    for t in threads: t.join()
    assert not failures, failures
    assert [v.shape[0] for v, _ in stubbed["stats"][0::2]] == [21, 40]  # 20 rounded up to the three ranks, then the cap
    assert [v.shape[0] for v, _, _ in stubbed["moments"][0::2]] == [21, 40]     # both calls once per round and output: rank 0 alone
    assert len(stubbed["stats"]) == len(stubbed["moments"]) == 4
    for r in range(size):
        assert sum(n for _, n in type(problems[r]).calls) == (14 if r == 0 else 13)     # 7 each, then 19 = 7 + 6 + 6
        assert problems[r].pilot_report == problems[0].pilot_report and problems[r].pilot_report["capped_by"] == "samples"
        assert np.array_equal(_bits(problems[r].get_covariances()), _bits(problems[0].get_covariances()))
        assert np.array_equal(problems[r].get_covariance_error(1), problems[0].get_covariance_error(1))
    field = stubbed["stats"][-2][0]                                     # the number: round-major, then in rank order
    first_of = lambda rank, call: 2.0 + np.random.default_rng(1000 * rank + call).standard_normal((4, 3)) @ MIX[0]      # (a batch of four)
    assert field[0, 0, 0] == first_of(0, 1)[0] and field[7, 0, 0] == first_of(1, 1)[0] and field[14, 0, 0] == first_of(2, 1)[0]
    assert field[21, 0, 0] == first_of(0, 3)[0] and field[28, 0, 0] == first_of(1, 3)[0] and field[34, 0, 0] == first_of(2, 3)[0]


# ---- refusals -----------------------------------------------------------------------------------------------------------------------
def test_python_inner_products_behave_as_the_bases_and_refuse_a_tolerance(stubbed):
    from bluest_amd.sap import BLUESTError
    E, F, PM, B = _classes()

    def own(self):
        return [lambda a, b: a * b, lambda a, b: float(np.dot(a * MASS, b))]
    cls = _seeded_class(E, F, PM, B)
    cls.get_models_inner_products = own
    p = cls(M, costs=[4.0, 2.0, 1.0], n_outputs=2, covariance_estimation_samples=20, sample_batch_size=4, verbose=False, skip_projection=True)
    ref_cls = _seeded_class(F, PM, B)
    ref_cls.get_models_inner_products = own
    q = ref_cls(M, costs=[4.0, 2.0, 1.0], n_outputs=2, covariance_estimation_samples=20, sample_batch_size=4, verbose=False, skip_projection=True)
    assert stubbed["moments"] == [] and p.pilot_report is None
    assert np.array_equal(_bits(p.get_covariances()), _bits(q.get_covariances()))
    for call in (p.get_covariance_errors, p.get_covariance_error, p.get_mlmc_variance_errors, p.get_mlmc_variance_error):
        with pytest.raises(BLUESTError, match="inner products"):
            call()
    with pytest.raises(BLUESTError, match="inner products"):
        cls(M, costs=[4.0, 2.0, 1.0], n_outputs=2, covariance_estimation_tol=0.1, verbose=False)


def test_without_fieldoutputsmixin_a_tolerance_is_refused():
    from bluest_amd.sap import BLUESTError
    E, F, PM, B = _classes()

    class P(E, PM, B):
        def sampler(self, ls, N=1): pytest.fail("refused before anything is drawn")

    with pytest.raises(BLUESTError, match="FieldOutputsMixin"):
        P(2, costs=[2.0, 1.0], covariance_estimation_tol=0.1, verbose=False)
    with pytest.raises(ValueError):
        _make(E, F, PM, B, covariance_estimation_tol=-1.0)


def test_pilot_errors_mixin_still_refuses_fields():
    from bluest_amd.pilot_errors import PilotErrorsMixin
    from bluest_amd.sap import BLUESTError
    E, F, PM, B = _classes()

    class P(PilotErrorsMixin, F, PM, B):
        def sampler(self, ls, N=1): pytest.fail("refused before anything is drawn")

    with pytest.raises(BLUESTError, match="FieldOutputsMixin"):
        P(2, costs=[2.0, 1.0], covariance_estimation_tol=0.1, verbose=False)


def test_a_loaded_problem_has_no_errors_and_refuses_a_tolerance():
    from bluest_amd.sap import BLUESTError
    E, F, PM, B = _classes()

    class P(E, F, PM, B):
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
    with pytest.raises(BLUESTError):                                    # sample files stay refused
        _make(E, F, PM, B, samplefile="samples.npz")


def test_nothing_unknown_means_nothing_has_an_error(stubbed):
    E, F, PM, B = _classes()

    class P(E, F, PM, B):
        def output_weights(self): return [MASS]
        def sampler(self, ls, N=1): pytest.fail("nothing is unknown: nothing to sample")

    C = np.array([[2.0, 0.5, np.inf], [0.5, 1.0, 0.25], [np.inf, 0.25, 1.5]])
    p = P(3, C=C, costs=[4.0, 2.0, 1.0], covariance_estimation_tol=0.1, verbose=False)
    assert np.isnan(p.get_covariance_error()).all() and np.isnan(p.get_mlmc_variance_error()).all()
    assert p.pilot_report == {"samples": 0, "rounds": 0, "ratio": None, "converged": True, "capped_by": None} and stubbed["moments"] == []

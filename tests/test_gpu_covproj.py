"""GPU tests of the SPD covariance projection (BLUEProblem.project_covariance(s), bluest_cov_project): against the reference
fixtures of tools/gen_golden_covproj.py, and oracle-free optimality checks of the SPG result."""
import contextlib
import glob
import io
import os

import numpy as np
import pytest

import covproj_cases as cc
from bluest_amd.blue_models import cov_project, spg_default_params
from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(p)[len("covproj_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "covproj_*_M*.npz")))
THR = 5.0e-14


def _problem(g):
    from bluest_amd.blue_models import BLUEProblem
    Cs = [c.copy() for c in g["C"]]
    params = {"verbose": bool(g["verbose"]), "remove_uncorrelated": bool(g["remove_uncorrelated"]),
              "skip_projection": bool(g["skip_projection"])}
    if int(g["maxit"]) >= 0:
        params["spg_params"] = {"maxit": int(g["maxit"])}
    return BLUEProblem(Cs[0].shape[0], C=Cs, costs=g["costs"].copy(), n_outputs=len(Cs), **params)


def _run(g):
    """what the generator did, on this build: (covariances afterwards, returned errors, captured stdout)"""
    out = io.StringIO()
    n_out = g["C"].shape[0]
    err = np.full(n_out, np.nan)
    with contextlib.redirect_stdout(out):
        p = _problem(g)
        if int(g["call"]) == 0:
            for n in range(n_out):
                err[n] = p.project_covariance(n, bypass_error_check=bool(g["bypass"]))
    return np.array(p.get_covariances()), err, out.getvalue()


def _np_proj(X):
    l, V = np.linalg.eigh((X + X.T) / 2)
    return (V * np.maximum(l, THR)) @ V.T


def _check_optimal(X, C, mask):
    """X minimises 1/2 ||mask o (X - C)||^2 over {X = X^T, lambda_min >= THR}: feasible, and a fixed point of the projected
    gradient step.  lambda_min is judged to within the accuracy of a float64 matrix, 64 eps ||X||_2: at an optimum the clip is
    active, so the smallest eigenvalues sit at THR and rounding moves them by ~eps ||X||, far more than THR * 1e-9."""
    scale = np.abs(np.where(mask > 0, C, 0.0)).max()
    assert np.array_equal(X, X.T)
    lam = np.linalg.eigvalsh(X)
    assert lam[0] >= THR * (1 - 1e-9) - 64 * np.finfo(float).eps * lam[-1], (lam[0], lam[-1])
    g = mask * (X - np.where(mask > 0, C, 0.0))
    assert np.abs(X - _np_proj(X - g)).max() <= 1e-9 * scale


@pytest.mark.parametrize("name", CASES)
def test_projection_matches_reference_fixture(name):
    g = golden("covproj_%s.npz" % name)
    if int(g["raises"]):
        with pytest.raises(RuntimeError, match="Could not find good enough Covariance projection"):
            _run(g)
        return
    cov, err, stdout = _run(g)
    ref = g["cov"]
    for n in range(ref.shape[0]):
        scale = np.abs(g["C"][n][np.isfinite(g["C"][n])]).max()
        assert np.array_equal(np.isnan(cov[n]), np.isnan(ref[n])), (name, n)
        assert np.array_equal(cov[n] == 0.0, ref[n] == 0.0), (name, n)
        known = ~np.isnan(ref[n])
        assert np.abs(cov[n][known] - ref[n][known]).max() <= 1e-8 * scale, (name, n, np.abs(cov[n][known] - ref[n][known]).max())
        if int(g["call"]) == 0:
            e, er = err[n], g["err"][n]
            if bool(g["finite"][n]):
                assert abs(e - er) <= 1e-12 * abs(er), (name, n, e, er)
            else:
                # the SPG objective; below (eps)^2 * M^2 * scale^2 both solves are at the optimum, where f is rounding noise
                assert abs(e - er) <= 1e-8 * abs(er) + (1e-10 * g["C"].shape[1] * scale) ** 2, (name, n, e, er)
    # the trajectory, not only its end: the kernel's it and count are the reference's, on the fixtures whose decisions the
    # longdouble restatement finds safe (covproj_cases.FIXTURE_MARGINAL names the two that are not).  Every output is handed
    # to the kernel as project_covariance hands it over, whether the fixture projected by a call or in the constructor.
    if name not in cc.FIXTURE_MARGINAL:
        for n in range(ref.shape[0]):
            C, mask, params = cc.fixture_inputs(g, n)
            (_, _, _, it, count, info), = cov_project([C], [mask], dict(spg_default_params, **params))
            want = (0, 0) if bool(g["finite"][n]) else (int(g["it"][n]), int(g["count"][n]))
            assert info == 0 and (it, count) == want, (name, n, it, count, want)
    if bool(g["verbose"]):
        warned = "WARNING! Large covariance projection error" in stdout
        assert warned == ("WARNING! Large covariance projection error" in str(g["stdout"]))


def _partial_indefinite(M, seed, frac=0.2, neg=0.1):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(M, M))
    l = rng.uniform(0.2, 2.0, M)
    l[:3] = -neg * rng.uniform(0.5, 1.0, 3)
    C = Q @ np.diag(l) @ Q.T
    C = (C + C.T) / 2
    mask = np.ones((M, M))
    for i in range(1, M):
        for j in range(i + 1, M):
            if rng.rand() < frac:
                mask[i, j] = mask[j, i] = 0.0
    return np.where(mask > 0, C, np.nan), mask


def _spg(Cs, masks, **over):
    return cov_project([np.where(m > 0, c, 0.0) for c, m in zip(Cs, masks)], masks, dict(spg_default_params, **over))


def test_spg_results_are_optimal_on_every_fixture():
    for name in CASES:
        g = golden("covproj_%s.npz" % name)
        if int(g["raises"]):
            continue
        for n in range(g["C"].shape[0]):
            C = g["C"][n]
            mask = (~np.isinf(C)).astype(np.float64)
            if int(g["call"]) == 0 and bool(g["remove_uncorrelated"]):
                mask[C == 0] = 0.0
            np.fill_diagonal(mask, 1.0)
            if mask.all():
                continue
            (X, f, gpmax, it, count, info), = _spg([C], [mask])
            assert info == 0 and gpmax <= 1e-10 and it >= 0 and count >= 1, (name, n, info, gpmax)
            _check_optimal(X, C, mask)
            r = mask * (X - np.where(mask > 0, C, 0.0))
            assert abs(f - 0.5 * (r * r).sum()) <= 1e-12 * max(f, 1e-300) + 1e-28


@pytest.mark.parametrize("n_out", [1, 4])
def test_m64_lds_worst_case(n_out):
    Cs, masks = zip(*[_partial_indefinite(64, 640 + o) for o in range(n_out)])
    res = _spg(Cs, masks)
    for (X, f, gpmax, it, count, info), C, mask in zip(res, Cs, masks):
        assert info == 0 and gpmax <= 1e-10, (info, gpmax, it)
        _check_optimal(X, C, mask)
    # the single clip at M = 64: against LAPACK
    C = np.nan_to_num(Cs[0], nan=0.0)
    C = (C + C.T) / 2
    (X, f, _, it, _, info), = _spg([C], [np.ones((64, 64))])
    l, V = np.linalg.eigh(C)
    ref = (V * np.maximum(l, THR)) @ V.T
    assert info == 0 and it == 0
    assert np.abs(X - ref).max() <= 1e-12 * np.abs(C).max()
    assert abs(f / np.linalg.norm(C - ref) - 1) <= 1e-12


def test_one_and_two_models():
    from bluest_amd.blue_models import BLUEProblem
    p = BLUEProblem(1, C=np.array([[-0.5]]), costs=[1.0], verbose=False)
    assert p.project_covariance() == pytest.approx(0.5 + THR, rel=1e-15)
    assert p.get_covariance()[0, 0] == pytest.approx(THR, rel=1e-12)
    C = np.array([[1.0, 2.0], [2.0, 1.0]])                               # eigenvalues -1 and 3
    p = BLUEProblem(2, C=C, costs=[2.0, 1.0], verbose=False)
    err = p.project_covariance()
    l, V = np.linalg.eigh(C)
    ref = (V * np.maximum(l, THR)) @ V.T
    assert np.abs(p.get_covariance() - ref).max() <= 1e-14 and abs(err / np.linalg.norm(C - ref) - 1) < 1e-12
    # two models, the pair not coupled, the second variance negative: the optimum is diag(1, THR), f = (0.5 + THR)^2 / 2
    p = BLUEProblem(2, C=np.array([[1.0, np.inf], [np.inf, -0.5]]), costs=[2.0, 1.0], verbose=False)
    err = p.project_covariance()
    got = p.get_covariance()
    assert np.isnan(got[0, 1]) and np.isnan(got[1, 0])
    assert abs(got[0, 0] - 1.0) <= 1e-12 and abs(got[1, 1] - THR) <= 1e-12
    assert err == pytest.approx(0.5 * (0.5 + THR) ** 2, rel=1e-8)


def test_verbose_early_return_leaves_covariance_and_bypass_updates_it():
    from bluest_amd.blue_models import BLUEProblem
    g = golden("covproj_early_return_M7.npz")
    C = g["C"][0]
    p = BLUEProblem(7, C=C.copy(), costs=g["costs"], verbose=True)
    before = p.get_covariance()
    out = io.StringIO()
    with contextlib.redirect_stdout(out):
        err = p.project_covariance()
    assert err > 1e-10 and "WARNING! Large covariance projection error" in out.getvalue()
    assert np.array_equal(p.get_covariance(), before, equal_nan=True)
    with contextlib.redirect_stdout(io.StringIO()):
        err2 = p.project_covariance(bypass_error_check=True)
    assert err2 == err
    after = p.get_covariance()
    assert not np.array_equal(after, before, equal_nan=True)
    assert np.array_equal(np.isnan(after), np.isnan(before))
    # not verbose: always updated
    q = BLUEProblem(7, C=C.copy(), costs=g["costs"], verbose=False)
    q.project_covariances()
    assert np.array_equal(q.get_covariance(), after, equal_nan=True)


def test_nonfinite_known_entry_is_a_status_not_a_fault():
    from bluest_amd.blue_models import BLUEST_COVPROJ_NONFINITE
    C = np.eye(3)
    C[0, 1] = C[1, 0] = 1e308 * 10
    (X, f, gpmax, it, count, info), = _spg([C], [np.ones((3, 3))])
    assert info == BLUEST_COVPROJ_NONFINITE and it == 0
    from bluest_amd import _lib
    with pytest.raises(_lib.BluestHipError, match="M=65"):
        _spg([np.eye(65)], [np.ones((65, 65))])


def test_setup_solver_is_certified_after_projecting_an_indefinite_pilot():
    from bluest_amd.blue_models import BLUEProblem
    g = golden("covproj_finite_M12.npz")
    C = g["C"][0]
    assert np.linalg.eigvalsh(C)[0] < 0
    p = BLUEProblem(12, C=C.copy(), costs=g["costs"], verbose=False)
    p.project_covariances()
    P = p.get_covariance()
    assert np.linalg.eigvalsh(P)[0] > 0
    budget = 100.0 * g["costs"][0]
    out = p.setup_solver(K=3, budget=budget, solver="spg", continuous_relaxation=True)
    assert out["total_cost"] <= budget * (1 + 1e-9)
    info = p.MOSAP.solver_info
    assert info["certified_gap"] <= 1e-8, info
    assert np.isfinite(out["errors"]).all() and (np.asarray(out["errors"]) > 0).all()

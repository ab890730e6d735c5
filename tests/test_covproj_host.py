"""CPU tests of the SPD covariance projection (BLUEProblem.project_covariance(s), include/bluest_hip.h Part 8): the C-ABI
declaration and binding, the new default parameters, and the integrity of the reference fixtures (tools/gen_golden_covproj.py)."""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

CASES = sorted(os.path.basename(p)[len("covproj_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "covproj_*_M*.npz")))


def test_cov_project_declared_and_bound():
    import ctypes
    from bluest_amd import _lib, build
    build.build()
    assert "bluest_cov_project" in _lib.SIGNATURES and len(_lib.SIGNATURES["bluest_cov_project"]) == 18
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bluest_cov_project")
    text = open(build.HDR).read()
    assert "Part 8" in text and "int bluest_cov_project(int M, int n_out, const double *C, const double *mask" in text
    for name, value in (("OK", 0), ("MAXIT", 1), ("MAXFEV", 2), ("NONFINITE", 3), ("NOEIG", 4)):
        assert ("#define BLUEST_COVPROJ_%s" % name) in text
        assert [ln.split()[2] for ln in text.splitlines() if ln.startswith("#define BLUEST_COVPROJ_%s " % name)] == [str(value)]
    assert "covproj.hip" in build.SOURCES


def test_default_params_gain_projection_keys():
    from bluest_amd import blue_models as bm
    assert bm.default_params["skip_projection"] is True
    assert bm.spg_default_params == {"maxit": 10000, "max_fevals": 10000**2, "verbose": False, "spd_threshold": 5.0e-14,
                                     "eps": 1.0e-10, "lmbda_min": 10.**-30, "lmbda_max": 10.**30, "linesearch_history_length": 10}
    assert bm.default_params["spg_params"] == bm.spg_default_params


def test_spg_params_are_merged_as_the_reference_merges_them():
    from bluest_amd import blue_models as bm
    C = np.array([[2.0, 0.5], [0.5, 1.0]])
    p = bm.BLUEProblem(2, C=C, costs=[2.0, 1.0], verbose=False, spg_params={"maxit": 3})
    assert p.params["spg_params"] == dict(bm.spg_default_params, maxit=3)
    assert bm.spg_default_params["maxit"] == 10000                   # the defaults themselves are not touched
    q = bm.BLUEProblem(2, C=C, costs=[2.0, 1.0], verbose=False)
    assert q.params["spg_params"] == bm.spg_default_params and q.params["skip_projection"] is True
    assert np.array_equal(q.get_covariance(), C)                     # default: the constructor leaves C as given


def test_only_project_covariances_leaves_the_refused_set():
    from bluest_amd import blue_models as bm
    from bluest_amd.sap import BLUESTError
    B = bm.BLUEProblem
    assert B.project_covariances is not B._out_of_scope and B.project_covariance is not B._out_of_scope
    for name in ("setup_mlmc", "solve_mlmc", "setup_mc", "save_graph_data", "load_graph_data", "estimate_missing_covariances",
                 "estimate_costs", "complexity_test", "variance_test"):
        assert getattr(B, name) is B._out_of_scope, name
    p = B(2, C=np.eye(2), costs=[2.0, 1.0], verbose=False)
    with pytest.raises(BLUESTError):
        p.setup_mc(budget=10.0)


def test_fixtures_are_complete_and_consistent():
    assert len(CASES) >= 12, CASES
    for name in ("finite_M5", "finite_M12", "finite_M20", "partial_M6", "partial_M12", "partial_M20", "three_outputs_M8",
                 "early_return_M7", "bypass_M7", "maxit3_M6", "constructor_M9"):
        assert name in CASES, name
    for name in CASES:
        g = golden("covproj_%s.npz" % name)
        C, cov = g["C"], g["cov"]
        n_out, M = C.shape[0], C.shape[1]
        assert C.shape == cov.shape == (n_out, M, M) and g["costs"].shape == (M,)
        assert g["err"].shape == g["it"].shape == g["count"].shape == g["finite"].shape == (n_out,)
        if int(g["raises"]):
            assert int(g["maxit"]) == 3
            continue
        for n in range(n_out):
            known = np.isfinite(cov[n])
            assert np.array_equal(known, known.T) and np.diag(known).all()
            Cn = cov[n][known]
            assert np.isfinite(Cn).all()
            if int(g["call"]) == 0:
                # project_covariance keeps which pairs are coupled: NaN exactly where the input had inf (or a dropped zero)
                given = C[n].copy()
                dropped = np.isinf(given) | ((given == 0) & bool(g["remove_uncorrelated"]))
                np.fill_diagonal(dropped, False)
                assert np.array_equal(~known, dropped), (name, n)
                if bool(g["finite"][n]):
                    assert int(g["it"][n]) == -1 and np.isfinite(g["err"][n])
                else:
                    assert int(g["it"][n]) >= 0 and int(g["count"][n]) >= 1
    # the verbose early return left the covariance as it was; bypass_error_check=True updated it
    e, b = golden("covproj_early_return_M7.npz"), golden("covproj_bypass_M7.npz")
    given = np.where(np.isinf(e["C"][0]), np.nan, e["C"][0])
    assert np.array_equal(e["cov"][0], given, equal_nan=True)
    assert e["err"][0] > 1e-10 and e["err"][0] == b["err"][0]
    assert not np.array_equal(b["cov"][0], given, equal_nan=True)
    assert "WARNING! Large covariance projection error" in str(e["stdout"])
    assert "WARNING! Large covariance projection error" not in str(b["stdout"])
    # the constructor path: the zero pairs were projected first, then dropped only where the projection left them uncorrelated
    c = golden("covproj_constructor_M9.npz")
    assert int(c["skip_projection"]) == 0 and int(c["it"][0]) > 0
    # the single clip replaces every entry, a known zero included
    z = golden("covproj_finite_zero_M6.npz")
    assert z["C"][0][2, 4] == 0.0 and np.isfinite(z["cov"][0][2, 4]) and z["cov"][0][2, 4] != 0.0


def test_more_than_64_models_is_refused_before_the_gpu():
    from bluest_amd import blue_models as bm
    from bluest_amd.sap import BLUESTError
    p = bm.BLUEProblem(65, C=np.eye(65), costs=np.linspace(2.0, 1.0, 65), verbose=False)
    with pytest.raises(BLUESTError, match="at most 64 models"):
        p.project_covariances()
    with pytest.raises(BLUESTError, match="at most 64 models"):
        bm.BLUEProblem(65, C=np.eye(65), costs=np.linspace(2.0, 1.0, 65), verbose=False, skip_projection=False)

"""CPU tests of the MFMC numpy mirrors (bluest_amd/misc.py, reference bluest/misc.py:48-130, 416-449) against reference fixtures
(tools/gen_golden_mfmc.py), and of the new C-ABI entry point's declaration."""
import numpy as np

from conftest import golden


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def test_attempt_mfmc_setup_matches_reference():
    from bluest_amd import misc
    g = golden("mfmc_helpers_tutorial.npz")
    C, w = g["C"], g["costs"]
    s = np.sqrt(np.diag(C))
    rho = (C / np.outer(s, s))[0]
    for k in range(int(g["n_attempts"])):
        cl, mode = g["a%d_clique" % k], str(g["a%d_mode" % k])
        kw = {"eps": dict(eps=0.01 * s[0]), "budget": dict(budget=100 * w.max()),
              "cont": dict(eps=0.01 * s[0], continuous_relaxation=True),
              "low": dict(budget=3.3 * w.max(), small_budget=True)}[mode]
        ok, d = misc.attempt_mfmc_setup(s[cl], rho[cl], w[cl], **kw)
        assert ok == bool(g["a%d_ok" % k]), (cl, mode)
        if not ok:
            continue
        ref = g["a%d_samples" % k]
        assert np.asarray(d["samples"]).dtype.kind == ref.dtype.kind
        if ref.dtype.kind == "i":
            assert np.array_equal(d["samples"], ref), (cl, mode)
        else:
            assert _rel(d["samples"], ref) < 1e-12
        assert _rel(d["error"], g["a%d_error" % k]) < 1e-12
        assert _rel(d["total_cost"], g["a%d_cost" % k]) < 1e-12
        assert _rel(d["alphas"], g["a%d_alphas" % k]) < 1e-12
        assert abs(np.sqrt(d["variance"](d["samples"])) / d["error"] - 1) < 1e-14


def test_low_budget_solution_matches_reference():
    from bluest_amd import misc
    g = golden("mfmc_helpers_tutorial.npz")
    C, w = g["C"], g["costs"]
    s = np.sqrt(np.diag(C))
    rho = (C / np.outer(s, s))[0]
    keys = [k for k in g if k.startswith("low")]
    assert keys
    for key in keys:
        cl = g["a%s_clique" % key[3:]]
        m = misc.mfmc_low_budget_integer_solution(rho[cl], w[cl], 3.3 * w.max())
        assert m.dtype == np.int64 and np.array_equal(m, g[key])


def test_compute_mfmc_data_matches_reference_fixture():
    from bluest_amd import misc
    for name in ("tutorial_eps", "n8_eps", "graph_budget"):
        g = golden("mfmc_%s.npz" % name)
        C, w, cl = g["C"][0], g["costs"], g["models"]
        s = np.sqrt(np.diag(C))
        rho = (C / np.outer(s, s))[0]
        ok, d = misc.compute_mfmc_data(s[cl], rho[cl], w[cl], g["samples"])
        assert ok
        assert _rel(d["error"], g["cd_errors"][0]) < 1e-12
        assert _rel(d["total_cost"], g["cd_total_cost"]) < 1e-12


def test_integer_bounds_follow_reference_order():
    from bluest_amd import misc
    sol = np.array([1.0, 3.7, 2.2, 9.5])
    lb, ub, idx = misc.mfmc_integer_bounds(sol)
    assert list(idx) == [3, 1, 2, 0] and list(lb) == [9, 3, 2, 1] and list(ub) == [10, 4, 3, 1]
    assert list(misc.mfmc_round_from_combo(sol, 0b0101)) == [1, 3, 3, 10]


def test_mfmc_search_declared_and_bound():
    import ctypes
    from bluest_amd import _lib, build
    build.build()
    assert "bluest_mfmc_search" in _lib.SIGNATURES
    assert hasattr(ctypes.CDLL(_lib.LIB_PATH), "bluest_mfmc_search")
    text = open(build.HDR).read()
    assert "BLUEST_MFMC_MAX_NEIGHBOURS 30" in text and "BLUEST_MFMC_MAX_ROUND      24" in text

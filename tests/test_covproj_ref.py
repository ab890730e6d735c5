"""
CPU tests of oracle/covproj_ref.py, the numpy restatement of bluest_cov_project that test_gpu_covproj_abi.py compares the
kernel with: the restatement reproduces the recorded runs of the reference project (tests/golden/covproj_*_M*.npz, `it` and
`count` included), every decision it takes on every row of tests/covproj_cases.py is further from flipping than float64
rounding in the kernel can move it, and the table reaches every path of the kernel that an input can reach.
"""
import glob
import os

import numpy as np
import pytest

import covproj_cases as cc
from conftest import GOLDEN, golden
from oracle import covproj_ref as ref

FIXTURES = sorted(os.path.basename(p)[len("covproj_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "covproj_*_M*.npz")))
MARGINAL, fixture_inputs = cc.FIXTURE_MARGINAL, cc.fixture_inputs


@pytest.mark.parametrize("name", FIXTURES)
def test_reference_reproduces_the_recorded_reference(name):
    g = golden("covproj_%s.npz" % name)
    for n in range(g["C"].shape[0]):
        C, mask, params = fixture_inputs(g, n)
        R = ref.run_ld(C, mask, params)
        scale = np.abs(C).max()
        if int(g["raises"]):                                          # maxit = 3: the reference raised, nothing recorded
            assert R.info == ref.MAXIT and R.it == 3
            continue
        assert R.info == ref.OK
        known = ~np.isnan(g["cov"][n])
        updated = not (bool(g["verbose"]) and not bool(g["bypass"]) and not bool(g["finite"][n]) and float(R.f) > 1e-10)
        if bool(g["finite"][n]):
            # LAPACK's eigh is backward stable with a constant of the same kind as the Jacobi bound: the same bound
            assert R.it == 0 and R.count == 0
            err = np.abs(R.X - g["cov"][n])
            print(name, n, "clip: max |X - cov| / bound = %.3g" % float((err / R.eX).max()))
            assert (err <= R.eX).all()
            assert abs(float(R.f) - g["err"][n]) <= float(np.sqrt((R.eX ** 2).sum())) + 4 * ref.U * g["err"][n]
            continue
        if name not in MARGINAL:
            assert (R.it, R.count) == (int(g["it"][n]), int(g["count"][n])), (name, n)
        else:
            print(name, n, "marginal: it %d (recorded %d), count %d (recorded %d), %d decisions inside their bound"
                  % (R.it, g["it"][n], R.count, g["count"][n], len(ref.margins_hold(R.decisions))))
            assert ref.margins_hold(R.decisions)
        # Two SPG runs that stop at gpmax <= 1e-10 agree to the stopping tolerance, not to rounding: 100 times the stopping
        # tolerance, relative to the input, as test_gpu_covproj.py judges the kernel against the same fixtures.
        if updated:
            X = R.X.copy()
            sd = np.sqrt(np.diag(X))
            X[np.abs(X / np.outer(sd, sd)) < 1.0e-7] = 0.0
            assert np.abs(X[known] - g["cov"][n][known]).max() <= 1e-8 * scale
        if int(g["call"]) == 0:
            assert abs(float(R.f) - g["err"][n]) <= 1e-8 * g["err"][n] + (1e-10 * C.shape[0] * scale) ** 2


ROWS = [r["name"] for r in cc.all_cases()] + [b[0]["name"] for b in cc.budget_cases()] + [cc.overflow_case()["name"]]


@pytest.mark.parametrize("name", ROWS)
def test_every_decision_of_a_row_is_safe(name):
    R = cc.reference(name)
    assert R.rc == ref.RC_OK
    unsafe = ref.margins_hold(R.decisions)
    assert not unsafe, [(d[0], d[1], float(d[-2]), float(d[-1])) for d in unsafe]


def test_budget_rows_end_as_the_table_says():
    for row, info, it, count, exit_ in cc.budget_cases():
        R = cc.reference(row["name"])
        assert R.info == info, row["name"]
        assert it is None or R.it == it, row["name"]
        assert count is None or R.count == count, row["name"]
        assert exit_ is None or exit_ in R.paths, (row["name"], R.paths)
    for name, C, mask, info in cc.multi_case():
        assert ref.run_ld(C, mask, cc.MULTI_PARAMS).info == info, name


def test_the_table_reaches_every_path():
    reached = set()
    for name in ROWS:
        reached |= cc.reference(name).paths
    assert not [p for p in cc.REQUIRED if p not in reached]
    assert not [p for p in cc.UNREACHED if p in reached]
    assert reached <= set(cc.REQUIRED) | set(cc.UNREACHED)            # a path that neither list knows
    sizes = {r["C"].shape[0] for r in cc.by_group("spg")}
    assert sizes == set(cc.SPG_SIZES)
    assert {r["C"].shape[0] for r in cc.by_group("clip")} == set(cc.CLIP_SIZES)
    assert {r["params"].get("hlength", 10) for r in cc.by_group("spg")} >= {1, 2, 10, 64}
    # odd M above 7 in the SPG projection, and the lower_only clip at a size with a pad index
    assert any(r["C"].shape[0] == 13 for r in cc.by_group("spg"))
    assert "clip:lower_only" in cc.reference("clip_asymmetric_M63").paths
    # weights 0.5, 2, -1 and 1e-8 all occur, the last on an entry that is known and weighs nothing
    m = cc.case("spg_weights_M7")["mask"]
    assert {0.0, 0.5, 2.0, -1.0, 1e-8} <= set(np.unique(m))


def test_history_length_decides_a_nonmonotone_step():
    """hlength = 10 accepts at its first trial a step with f_new > f; hlength = 1, from the same point, rejects it"""
    a, b = cc.reference("spg_nonmonotone_M7_h10"), cc.reference("spg_nonmonotone_M7_h1")
    k = next(i for i, st in enumerate(a.steps) if "ls:nonmonotone" in st.paths and st.ntrial == 1)
    assert k >= 1 and all(np.array_equal(a.steps[i].x64, b.steps[i].x64) for i in range(k))
    assert b.steps[k].ntrial > 1


def test_proj_ld_against_lapack_and_its_own_properties():
    for M, seed in ((1, 0), (2, 1), (7, 2), (13, 3), (32, 4)):
        C = cc.indefinite(M, seed, nneg=max(1, M // 3))
        P, b = ref.proj_ld(C, 5e-14)
        l, V = np.linalg.eigh(C)
        assert (np.abs(P - (V * np.maximum(l, 5e-14)) @ V.T) <= b).all()
        assert np.array_equal(P, P.T)
        P2, _ = ref.proj_ld(P, 5e-14)                                 # idempotent to longdouble rounding
        assert np.abs(P2 - P).max() <= 1e-17 * max(float(np.abs(P).max()), 1e-300)
        lo, _ = ref.proj_ld(np.tril(C) + np.triu(np.ones((M, M)), 1), 5e-14, lower_only=True)
        assert np.abs(lo - P).max() <= 1e-17 * float(np.abs(P).max())
    # the overflow input: far beyond where sum a^2 is finite in float64
    r = cc.overflow_case()
    assert not np.isfinite((r["C"] * r["C"]).sum())
    P, b = ref.proj_ld(r["C"], 5e-14, lower_only=True)
    l, V = np.linalg.eigh(r["C"] / 1e155)
    assert (np.abs(P / 1e155 - (V * np.maximum(l, 0)) @ V.T) <= b / 1e155).all()


def test_argument_checks():
    P = dict(ref.default_params)
    assert ref.check_args(1, 1, P) == ref.RC_OK and ref.check_args(64, 1024, P) == ref.RC_OK
    for M, n_out, change in ((0, 1, {}), (65, 1, {}), (3, 0, {}), (3, 1025, {}), (3, 1, {"hlength": 0}), (3, 1, {"hlength": 65}),
                             (3, 1, {"eps": float("nan")}), (3, 1, {"maxit": -1})):
        assert ref.check_args(M, n_out, dict(P, **change)) == ref.ERR_ARG

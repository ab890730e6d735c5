"""
CPU tests of the integer-projection case table and its 80-bit reference (tests/intproj_cases.py), which test_gpu_intproj.py holds
k_intproj<NT> to: the reference agrees with a plain float64 solve of the same matrices inside the tolerance it grants the kernel,
the table reaches every instantiation the library is built with, with N == NT and with N < NT, and every launch keeps the
builder's conditions (exact zeros for unsupported models, the eigenvalue margin of the indefinite candidates, no finite candidate
between "well-conditioned under the cap" and "ill-conditioned on purpose").
"""
import numpy as np
import pytest

import intproj_cases as ic

NTS = ic.nt_values()
TABLE = ic.table_n(NTS)


def test_table_covers_every_instantiation():
    """every NT of launch_sets()["nt"] is dispatched to with N == NT (clear_pads skipped) and with N < NT (pads), at every LL and
    at 1 and 3 outputs; the widest NT also at 16.  A new NT without a case, or an N taken out of the table, fails here"""
    from bluest_amd.plan import launch_sets
    nts = sorted(launch_sets()["nt"])
    assert nts == NTS
    full, padded = set(), set()
    for N in TABLE:
        (full if ic.nt_of(N, nts) == N else padded).add(ic.nt_of(N, nts))
        got = {(L["LL"], L["n_out"], L["variant"]) for L in ic.launches(N, nts)}
        for LL in ic.LLS:
            for n_out in (1, 3):
                assert (LL, n_out, "full") in got and (LL, n_out, "nom0") in got
                assert ((LL, n_out, "sparse") in got) == (N >= 4) and ((LL, n_out, "ill") in got) == (N >= 2)
            assert ((LL, 16, "full") in got) == (N == nts[-1])
    assert full == set(nts) and padded == set(nts), (sorted(full), sorted(padded))
    assert 1 in TABLE and 2 in TABLE and max(TABLE) == nts[-1]
    # each N between two instantiations is the smallest that the upper one takes: the most pads
    for lo, hi in zip([0] + nts[:-1], nts):
        assert lo + 1 in TABLE and ic.nt_of(lo + 1, nts) == hi


@pytest.mark.parametrize("N", TABLE)
def test_builder_conditions(N):
    kinds = set()
    for L in ic.launches(N, NTS):
        refs = ic.reference(L)                          # asserts that no (candidate, output) is a judgement call
        n = L["N"]
        assert L["base"].shape == (L["n_out"], n * n) and L["cols"].shape == (L["n_out"], L["LL"], n * n)
        assert L["ms"].shape[1] == L["LL"] and L["base"].dtype == L["cols"].dtype == L["ms"].dtype == np.float64
        for o in range(L["n_out"]):
            # exact zeros in base and in every column for a model that is in no group; inputs symmetric bit for bit
            for M in [L["base"][o]] + list(L["cols"][o]):
                M = M.reshape(n, n)
                assert np.array_equal(M, M.T)
                for a in L["absent"]:
                    assert not M[a].any() and not M[:, a].any()
            assert [bool(L["cols"][o, j].any()) for j in range(L["LL"])] == [bool(x) and len(L["free"][j]) > 0
                                                                            for j, x in enumerate(L["in_out"][o])]
        if L["n_out"] > 1:
            assert not L["in_out"].all() and L["in_out"][0].all()      # some output lacks some free group
        for c, row in enumerate(refs):
            kind = L["kinds"][c]
            for o, r in enumerate(row):
                phi = ic.phi64(L, c, o)
                d = np.diag(phi)
                live = np.array([a not in L["absent"] for a in range(n)])
                assert (d[live] > 0).all() and not d[~live].any(), (N, L["variant"], kind, o)
                assert np.array_equal(r["sup"], np.flatnonzero(live))
                kinds.add((L["variant"], kind, r["kind"]))
                if L["variant"] == "nom0":
                    assert r["kind"] == ic.NOM0 and r["V"] == np.inf
                    continue
                if r["kind"] == ic.SING:
                    assert kind == "indefinite" and r["V"] == np.inf
                    A = phi[np.ix_(r["sup"], r["sup"])]
                    assert np.linalg.eigvalsh(A)[0] < -ic.INDEF_MARGIN * np.abs(A).max()
                    continue
                assert r["kind"] == ic.OK and np.isfinite(r["V"]) and r["V"] > 0
                if r["cond"] <= ic.COND_WELL:
                    assert r["derived"] <= ic.CAP and r["tol"] == r["derived"], (N, L["variant"], kind, o, r["cond"], r["derived"])
                else:
                    assert r["cond"] <= ic.COND_MAX and r["tol"] == r["derived"] < 1e-3
                if L["variant"] == "ill":
                    assert r["cond"] > ic.COND_WELL
                elif kind in ("dense", "zero"):
                    assert r["cond"] <= 1e3
            if kind == "indefinite":
                assert any(r["kind"] == ic.SING for r in row)
            if kind == "zero":
                assert not L["ms"][c].any()
            if kind == "large":
                assert L["ms"][c].max() == ic.LARGE and (L["LL"] == 1 or (L["ms"][c] != np.round(L["ms"][c])).any())
    want = {("full", "dense", ic.OK), ("full", "zero", ic.OK), ("full", "large", ic.OK), ("nom0", "dense", ic.NOM0),
            ("nom0", "zero", ic.NOM0)}
    if N >= 2:
        want |= {("full", "indefinite", ic.SING), ("ill", "dense", ic.OK), ("ill", "zero", ic.OK)}
    if N >= 4:
        want |= {("sparse", "dense", ic.OK), ("sparse", "zero", ic.OK), ("sparse", "large", ic.OK)}
    assert want <= kinds, want - kinds


@pytest.mark.parametrize("N", TABLE)
def test_reference_against_float64(N):
    """pinv of the float64 Phi gives [0, 0] within tol_V of the longdouble reference on every finite well-conditioned candidate
    (unsupported models are zero rows and columns of Phi: the pseudo-inverse of the padded matrix is the padded inverse)"""
    seen = 0
    worst = 0.0
    for L in ic.launches(N, NTS):
        for c, row in enumerate(ic.reference(L)):
            for o, r in enumerate(row):
                if r["kind"] != ic.OK or r["cond"] > ic.COND_WELL:
                    continue
                V = np.linalg.pinv(ic.phi64(L, c, o), hermitian=True)[0, 0]
                err = abs(V / r["V"] - 1)
                worst = max(worst, err / r["tol"])
                assert err <= r["tol"], (N, L["LL"], L["n_out"], L["variant"], L["kinds"][c], o, err, r["tol"])
                seen += 1
    print("N = %d: %d candidates, worst error / bound %.3f" % (N, seen, worst))
    assert seen >= 6 * 3


def test_reference_flags():
    """the three outcomes on matrices small enough to check by hand"""
    one = lambda base, col, m: ic.reference_one(2, np.array(base, float).ravel(), np.array([col], float).reshape(1, 4), [m])   # noqa: E731
    r = one([[2, 1], [1, 2]], [[0, 0], [0, 1]], 1.0)              # [[2, 1], [1, 3]]^-1 [0, 0] = 3 / 5
    assert r["kind"] == ic.OK and abs(r["V"] - 0.6) < 1e-17 and list(r["sup"]) == [0, 1]
    r = one([[2, 0], [0, 0]], [[0, 0], [0, 0]], 3.0)              # model 1 unsupported: 1 / 2
    assert r["kind"] == ic.OK and r["V"] == 0.5 and list(r["sup"]) == [0]
    r = one([[0, 0], [0, 2]], [[0, 0], [0, 1]], 1.0)              # model 0 unsupported
    assert r["kind"] == ic.NOM0 and r["V"] == np.inf
    r = one([[0, 0], [0, 0]], [[0, 0], [0, 0]], 1.0)              # nothing supported
    assert r["kind"] == ic.NOM0 and r["V"] == np.inf
    r = one([[1, 2], [2, 1]], [[0, 0], [0, 0]], 1.0)              # positive diagonal, eigenvalues 3 and -1
    assert r["kind"] == ic.SING and r["V"] == np.inf
    with pytest.raises(AssertionError):
        one([[1, 0], [0, 1]], [[0, 0], [0, 1]], -1.0)             # a diagonal entry cancelled to zero: not a case the table may hold

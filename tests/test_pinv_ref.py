"""
CPU checks of the pseudo-inverse reference (pinv_ref.py) and of the case table (pinv_cases.py) that test_gpu_group_pinv.py and
test_gpu_record_pinv.py run on the GPU: the reference against closed forms and against mpmath at 40 digits, the admission
condition of every row (no eigenvalue near the cut-off, numpy's own float64 pinv inside the row's bound), and the table's coverage.
"""
import numpy as np
import pytest

import pinv_cases as pc
import pinv_ref as ref

LD = ref.LD
EPS_LD = float(np.finfo(LD).eps)


def _f64_pinv(B, delta=0.0):
    return np.linalg.pinv(ref.symmetrise(B) + delta * np.eye(len(B)), hermitian=True)


def _mpf(mp, x):
    """a longdouble as an mpf, exactly: its float64 rounding plus the remainder, which float64 holds too"""
    hi = float(x)
    return mp.mpf(hi) + mp.mpf(float(x - LD(hi)))


# ---- the reference against closed forms -----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [1, 2, 5, 16, 17, 32])
def test_diagonal_block_gives_exact_reciprocals(k):
    d = pc.block("diag", k, 0).diagonal()
    P, w, V = ref.pinv_ld(np.diag(d))
    assert np.array_equal(P, np.diag(LD(1) / d.astype(LD)))
    assert np.array_equal(w, d.astype(LD)) and np.array_equal(V, np.eye(k, dtype=LD))


@pytest.mark.parametrize("k", [2, 3, 8, 16, 17, 32])
def test_constant_block_is_ones_over_c_k_squared(k):
    c = 1.7
    P, w, _ = ref.pinv_ld(np.full((k, k), c))
    want = np.full((k, k), LD(1) / (LD(c) * k * k))
    assert ref.fro_err(P, want) <= 8 * k * EPS_LD
    assert ref.kept(w).sum() == 1 and ref.margins(w)[1] <= pc.DROPPED_MAX


def test_two_by_two_known_answers():
    P, _, _ = ref.pinv_ld(np.array([[2.0, 1.0], [1.0, 2.0]]))
    assert ref.fro_err(P, np.array([[2, -1], [-1, 2]], dtype=LD) / LD(3)) <= 8 * EPS_LD
    P, _, _ = ref.pinv_ld(np.array([[1.0, 1.0], [1.0, 1.0]]))              # singular: ones / 4
    assert ref.fro_err(P, np.full((2, 2), LD(0.25))) <= 8 * EPS_LD
    P, w, _ = ref.pinv_ld(np.array([[0.0, 1.0], [1.0, 0.0]]))              # indefinite: its own inverse, eigenvalues +-1
    assert ref.fro_err(P, np.array([[0, 1], [1, 0]], dtype=LD)) <= 8 * EPS_LD and sorted(float(x) for x in w) == [-1.0, 1.0]
    P, _, _ = ref.pinv_ld(np.array([[1.0, 3.0], [1.0, 1.0]]))              # asymmetric: the symmetrised [[1, 2], [2, 1]]
    assert ref.fro_err(P, np.array([[-1, 2], [2, -1]], dtype=LD) / LD(3)) <= 8 * EPS_LD


def test_block_diagonal_matrix_gives_the_blocks_answers():
    blocks = [pc.block("wishart", 5, 0), pc.block("dup1", 4, 1), pc.block("indefinite", 7, 0), pc.block("graded4", 3, 0)]
    n = sum(len(b) for b in blocks)
    M, want, o = np.zeros((n, n)), np.zeros((n, n), dtype=LD), 0
    for b in blocks:
        M[o:o + len(b), o:o + len(b)] = b
        want[o:o + len(b), o:o + len(b)] = ref.pinv_ld(b)[0]
        o += len(b)
    got, w, _ = ref.pinv_ld(M)
    assert ref.fro_err(got, want) <= 64 * n * ref.cond_kept(w) * EPS_LD


def test_unsorted_group_is_the_permuted_sorted_answer():
    for K in (2, 8, 16, 17, 32):
        B = pc.block("unsorted", K, 0)
        perm = np.random.RandomState(K).permutation(K)
        got = ref.pinv_ld(B[np.ix_(perm, perm)])[0]
        want = ref.pinv_ld(B)[0][np.ix_(perm, perm)]
        assert ref.fro_err(got, want) <= 64 * K * ref.cond_kept(ref.jacobi_eigh(B)[0]) * EPS_LD, K


@pytest.mark.parametrize("k", [3, 16, 32])
def test_reference_against_mpmath_at_40_digits(k):
    """the 80-bit pseudo-inverse against mpmath.eigsy at 40 digits with the same rule: its own error is at most a thousandth of
    the bound it serves as a reference for"""
    mp = pytest.importorskip("mpmath")
    mp.mp.dps = 40
    for kind in (("wishart", "graded8", "dup2") if k == 32 else ("wishart", "graded8", "dup2" if k >= 4 else "dup1", "rank1", "indefinite", "asym")):
        r = pc.block_reference(kind, k, 0)
        S = ref.symmetrise(r["B"])
        w, Q = mp.eigsy(mp.matrix(S.tolist()))
        wmax = max(abs(x) for x in w)
        inv = [1 / x if abs(x) > mp.mpf(ref.CUT) * wmax else mp.mpf(0) for x in w]
        assert sum(1 for x in inv if x != 0) == int(ref.kept(r["w"]).sum()), (k, kind)
        P = Q * mp.diag(inv) * Q.T
        num = mp.sqrt(sum((_mpf(mp, r["pinv"][i, j]) - P[i, j]) ** 2 for i in range(k) for j in range(k)))
        den = mp.sqrt(sum(P[i, j] ** 2 for i in range(k) for j in range(k)))
        err = float(num / den)
        print("k=%d %s: 80-bit reference against mpmath %.2e (bound of the case %.2e)" % (k, kind, err, r["tol"]))
        assert err <= 1e-3 * r["tol"], (k, kind, err)


# ---- admission of every row -----------------------------------------------------------------------------------------------------

def _admit(w, what):
    lo, hi = ref.margins(w)
    assert lo >= pc.KEPT_MIN, (what, "kept eigenvalue too close to the cut", lo)
    assert hi <= pc.DROPPED_MAX, (what, "dropped eigenvalue too close to the cut", hi)


@pytest.mark.parametrize("K", pc.KS)
def test_every_block_row_is_admissible(K):
    """no eigenvalue of the 80-bit decomposition between 1e-18 and 1e-10 of the largest, and numpy.linalg.pinv in float64 alone
    inside the row's bound: a row that fails is replaced in the table, not loosened here"""
    worst = 0.0
    for kind in pc.kinds_of(K):
        for rep in range(pc.REPS):
            r = pc.block_reference(kind, K, rep)
            _admit(r["w"], (kind, K, rep))
            err = ref.fro_err(_f64_pinv(r["B"]), r["pinv"])
            worst = max(worst, err / r["tol"])
            assert err <= r["tol"], (kind, K, rep, err, r["tol"])
            if r["exact"] is not None:
                assert ref.fro_err(r["exact"], r["pinv"]) <= ref.EPS, (kind, K, rep)      # the closed form, rounded to float64
    print("K=%d: numpy's largest error / bound %.2e" % (K, worst))


@pytest.mark.parametrize("N", pc.RECORD_NS)
def test_every_record_row_is_admissible(N):
    """the same for every pass of every record row, with numpy's pinv put through the rule of k_pinv_from_record"""
    for launch in pc.LAUNCHES:
        for row in pc.launch_rows(N, launch):
            r = pc.record_reference(row.name)
            for w in r["w"]:
                _admit(w, row.name)
            if not r["w"]:
                assert row.kind in ("big0", "allzero") and not np.any(r["v"]), row.name
                assert (np.isinf(r["V"]) and r["status"] == ref.EVAL_INF) if row.kind == "big0" else \
                       (np.isnan(r["V"]) and r["status"] == ref.EVAL_NO_MODEL0), row.name
                continue
            rec, d = r["rec"], r["delta"]
            Phi, s1, s2 = rec[:N * N].reshape(N, N), rec[N * N:N * N + N] > 0, rec[N * N + N:N * N + 2 * N] > 0
            m2 = np.ones(N, dtype=bool) if d != 0.0 else s2

            def f64(mask):
                i = np.flatnonzero(mask)
                return i, _f64_pinv(Phi[np.ix_(i, i)], d)
            i1, P1 = f64(s1)
            assert ref.max_err(P1[0, 0], r["V"]) <= r["tolV"], row.name
            v = np.zeros(N)
            if m2[0]:
                i2, P2 = f64(m2)
                v[i2] = P2[0]
            assert ref.max_err(v, r["v"]) <= r["tolv"], row.name
            assert r["status"] == (ref.EVAL_OK if s1[0] else ref.EVAL_NO_MODEL0), row.name
            assert bool(np.any(r["v"])) == bool(m2[0]), row.name


# ---- coverage of the table ------------------------------------------------------------------------------------------------------

def test_block_table_reaches_every_size_type_and_kind():
    assert len(pc.BLOCK_ROWS) == pc.N_BLOCK_ROWS and len({r.name for r in pc.BLOCK_ROWS}) == pc.N_BLOCK_ROWS
    assert pc.KS == tuple(range(1, 33))
    for K in pc.KS:
        for index in pc.INDEX_TYPES:
            have = [r.kind for r in pc.rows_of(K, index)]
            for kind, kmin in pc.KINDS.items():
                assert have.count(kind) == (pc.REPS if K >= kmin else 0), (K, index, kind)
    for K in pc.COVERAGE_KS:
        assert set(pc.kinds_of(K)) == {k for k, kmin in pc.KINDS.items() if K >= kmin}
    assert set(pc.kinds_of(4)) == set(pc.KINDS) and len(pc.KINDS) == 10
    assert set(pc.SCALE_KS) == {2, 8, 16, 17, 32} and pc.SCALES == (515, -540)
    assert set(pc.NARROW_EDGES) == {1, 8, 16} and all(v == (1, 63, 64, 65, 200) for v in pc.NARROW_EDGES.values())
    assert set(pc.WIDE_EDGES) == {17, 32} and all(v == (1, 2, 65) for v in pc.WIDE_EDGES.values())
    assert pc.BIG_N == 300 and pc.BIG_KS == (2, 16, 17, 32)


@pytest.mark.parametrize("K", [1, 2, 7, 16, 17, 32])
def test_calls_hold_the_blocks_they_name(K):
    """every call: at most 64 models, every group owns its models, C[g, g] is the row's block and only "unsorted" groups are
    unsorted; both index types get the same blocks"""
    for index in pc.INDEX_TYPES:
        calls = pc.calls_of(K, index)
        assert sum(len(c.rows) for c in calls) == len(pc.rows_of(K, index))
        for c in calls:
            assert c.C.shape[0] <= 64 and c.groups.min() >= 0 and c.groups.max() < c.C.shape[0]
            assert len(np.unique(c.groups)) == c.groups.size
            for g, row, B in zip(c.groups, c.rows, c.blocks):
                assert np.array_equal(c.C[np.ix_(g, g)], B) and np.array_equal(B, pc.row_reference(row)["B"])
                assert (row.kind == "unsorted") == (K > 1 and not (np.diff(g) > 0).all()), row.name
    for K2 in pc.BIG_KS:
        C, g = pc.big_index_case(K2)
        assert C.shape == (300, 300) and g.max() == 299 and g[0].min() >= 256 and all(len(set(x)) == K2 for x in g)


def test_record_table_reaches_every_case():
    assert len(pc.RECORD_ROWS) == pc.N_RECORD_ROWS == 126 and len({r.name for r in pc.RECORD_ROWS}) == 126
    assert pc.RECORD_NS == (1, 2, 5, 33, 54, 55, 64) and (pc.N_OUT, pc.N_CAND) == (3, 2)
    for N in pc.RECORD_NS:
        have = {r.kind for r in pc.RECORD_ROWS if r.N == N}
        for kind, nmin in pc.RECORD_KINDS.items():
            if N >= nmin and not (kind == "spd_delta" and N >= 5):
                assert kind in have, (N, kind)
        for launch in pc.LAUNCHES:
            rows = pc.launch_rows(N, launch)
            assert len(rows) == 6 and len({pc.record_reference(r.name)["delta"] for r in rows}) == 1, (N, launch)
            if N >= 5:                                     # different matrices in the six slots: an indexing slip shows
                recs = [pc.record_reference(r.name)["rec"] for r in rows]
                assert all(not np.array_equal(recs[i], recs[j]) for i in range(6) for j in range(i)), (N, launch)
    # what the singular two-pass rows are there for
    for N in (5, 33, 54, 55, 64):
        r = pc.record_reference("two_pass_singular_N%d_C0" % N)
        assert r["delta"] != 0.0 and len(r["w"]) == 2 and len(r["w"][0]) == N - 2 and len(r["w"][1]) == N
        r = pc.record_reference("null_unsampled_N%d_A4" % N)
        assert len(r["w"]) == 2 and (~ref.kept(r["w"][0])).sum() >= 1 and len(r["w"][1]) < N
        r = pc.record_reference("no_model0_singular_N%d_B0" % N)
        assert r["status"] == ref.EVAL_NO_MODEL0 and np.any(r["v"]) and (~ref.kept(r["w"][0])).sum() >= 1
        r = pc.record_reference("defhalf_N%d_A3" % N)
        assert (~ref.kept(r["w"][0])).sum() == N // 2
        r = pc.record_reference("def2_N%d_A2" % N)
        assert (~ref.kept(r["w"][0])).sum() == 2

"""
The case table of the pseudo-inverse tests, generated from seeds: the blocks fed to k_group_pinv<K, G> / k_group_pinv_wide<G>
(test_gpu_group_pinv.py) and the records fed to k_pinv_from_record (test_gpu_record_pinv.py).  test_pinv_ref.py checks on the CPU
that every row is admissible (no eigenvalue near the cut-off, numpy's own pinv inside the bound) and that the table reaches every
size, index type, kind and record case.

A block row: name, kind, K, rep, index ("int64": bluest_group_pinv, "uint8": a Plan built from the covariance), build() -> the K x K
float64 matrix the kernel sees, in the order of the group.  A record row: name, kind, N, build() -> (Phi, s1, s2, big, delta).
"""
import collections
import functools

import numpy as np

import pinv_ref as ref

C_BOUND = 100.0                  # error <= C_BOUND cond_kept eps: the constant of test_group_pinv_wide_vs_numpy
WISHART_TOL = 1e-12              # well-conditioned Wishart blocks: the tolerance of the tests before these
KEPT_MIN, DROPPED_MAX = 1e-10, 1e-18      # admission: kept eigenvalues >= KEPT_MIN max|l|, dropped ones <= DROPPED_MAX max|l|

KS = tuple(range(1, 33))
INDEX_TYPES = ("int64", "uint8")
WIDE_KMIN = 17
# kind -> smallest K that admits it
KINDS = collections.OrderedDict([("wishart", 1), ("graded4", 2), ("graded8", 2), ("dup1", 2), ("dup2", 4), ("rank1", 2),
                                 ("indefinite", 1), ("asym", 2), ("unsorted", 2), ("diag", 1)])
REPS = 2                         # blocks of each kind per K
COVERAGE_KS = (1, 2, 3, 8, 12, 13, 16, 17, 32)
SCALE_KS = (2, 8, 16, 17, 32)
SCALES = (515, -540)             # pinv(2^e C) == 2^-e pinv(C), bit for bit
NARROW_EDGES = {1: (1, 63, 64, 65, 200), 8: (1, 63, 64, 65, 200), 16: (1, 63, 64, 65, 200)}      # K -> Lk, blocks of 64 threads
WIDE_EDGES = {17: (1, 2, 65), 32: (1, 2, 65)}                                                     # one wavefront per group
BIG_N, BIG_KS = 300, (2, 16, 17, 32)                                                              # model indices beyond a byte

BlockRow = collections.namedtuple("BlockRow", "name kind K rep index build")
RecordRow = collections.namedtuple("RecordRow", "name kind N build")


# ---- blocks -------------------------------------------------------------------------------------------------------------------

def _seed(kind, K, rep):
    return 100003 * list(KINDS).index(kind) + 101 * K + rep


def _wishart(K, rng):
    A = rng.randn(K, 4 * K + 4)
    return A @ A.T / (4 * K + 4)


def _spectrum(K, lam, rng):
    Q, _ = np.linalg.qr(rng.randn(K, K))
    B = (Q * lam) @ Q.T
    return 0.5 * (B + B.T)


def _duplicate(B, src, dst):
    """model dst becomes an exact copy of model src: row and column copied, as test_group_pinv_wide_vs_numpy does"""
    B[dst, :] = B[src, :]
    B[:, dst] = B[:, src]
    B[dst, dst] = B[src, src]
    return B


def block(kind, K, rep):
    """the K x K matrix of one block row (what the kernel sees, in group order; only "asym" is not symmetric)"""
    assert K >= KINDS[kind], (kind, K)
    rng = np.random.RandomState(_seed(kind, K, rep))
    if kind in ("wishart", "unsorted"):
        return _wishart(K, rng)
    if kind in ("graded4", "graded8"):
        return _spectrum(K, np.logspace(0, -float(kind[-1]), K), rng)
    if kind == "dup1":
        return _duplicate(_wishart(K, rng), int(rng.randint(0, K - 1)), K - 1)
    if kind == "dup2":
        B = _wishart(K, rng)
        a, b = rng.choice(K - 2, 2, replace=False)
        return _duplicate(_duplicate(B, int(a), K - 1), int(b), K - 2)
    if kind == "rank1":
        return np.full((K, K), float(rng.uniform(0.5, 2.0)))
    if kind == "indefinite":
        lam = rng.uniform(0.5, 2.0, K)
        lam[0] = -rng.uniform(0.5, 1.0)
        return _spectrum(K, lam, rng)
    if kind == "asym":
        return _wishart(K, rng) + 1e-3 * rng.randn(K, K)
    if kind == "diag":
        return np.diag(rng.uniform(0.5, 2.0, K) * 10.0 ** rng.randint(-3, 4, K))
    raise ValueError(kind)


def closed_form(kind, B):
    """the exact float64 answer of the kinds that have one (compared bit for bit), else None"""
    if kind == "diag":
        return np.diag(1.0 / np.diag(B))
    return None


def kinds_of(K):
    return [kind for kind, kmin in KINDS.items() if K >= kmin]


def block_rows():
    rows = []
    for K in KS:
        for index in INDEX_TYPES:
            for kind in kinds_of(K):
                for rep in range(REPS):
                    rows.append(BlockRow("%s_K%d_%d_%s" % (kind, K, rep, index), kind, K, rep, index, functools.partial(block, kind, K, rep)))
    return rows


BLOCK_ROWS = block_rows()
N_BLOCK_ROWS = 1244              # pinned: a row taken out fails test_pinv_ref.py


def rows_of(K, index):
    return [r for r in BLOCK_ROWS if r.K == K and r.index == index]


Call = collections.namedtuple("Call", "C groups rows blocks")      # one launch: covariance (N, N), groups (Lk, K) int64, their rows


def calls_of(K, index, max_models=64):
    """the rows of (K, index) packed into as few covariances of at most 64 models as hold them: every group owns K models of its
    own (scattered by a random permutation, sorted within the group but for the "unsorted" kind, whose order is shuffled), the
    block is written into C[g, g] and the rest of C is asymmetric noise that no group may read."""
    rows = rows_of(K, index)
    per_call = max(1, max_models // K)
    out = []
    for c0 in range(0, len(rows), per_call):
        part = rows[c0:c0 + per_call]
        N = min(max_models, len(part) * K + 3)
        rng = np.random.RandomState(7919 * K + c0)
        C = 10.0 * rng.randn(N, N)
        perm = rng.permutation(N)
        groups, blocks = [], []
        for i, row in enumerate(part):
            g = np.sort(perm[i * K:(i + 1) * K])
            if row.kind == "unsorted":
                while K > 1 and (np.diff(g) > 0).all():
                    g = rng.permutation(g)
            B = row.build()
            C[np.ix_(g, g)] = B
            groups.append(g)
            blocks.append(B)
        out.append(Call(C, np.array(groups, dtype=np.int64).reshape(len(part), K), part, blocks))
    return out


@functools.lru_cache(maxsize=None)
def block_reference(kind, K, rep):
    """dict of one block (shared by both index types): pinv (longdouble), w, cond, tol, closed form"""
    B = block(kind, K, rep)
    P, w, _ = ref.pinv_ld(B)
    cond = ref.cond_kept(w)
    tol = WISHART_TOL if kind in ("wishart", "unsorted") else C_BOUND * cond * ref.EPS
    return {"B": B, "pinv": P, "w": w, "cond": cond, "tol": tol, "exact": closed_form(kind, B)}


def row_reference(row):
    return block_reference(row.kind, row.K, row.rep)


def edge_pool(K, n=5):
    """(C, pool): a covariance of at most 64 models and n distinct sorted groups of K models in it (Wishart blocks, or fewer
    groups where 64 models do not hold n), for the launch-edge tests: a call of Lk groups repeats the pool cyclically"""
    n = min(n, max(1, 64 // K))
    rng = np.random.RandomState(31 * K + 5)
    N = min(64, n * K + 2)
    C = 10.0 * rng.randn(N, N)
    perm = rng.permutation(N)
    pool = []
    for i in range(n):
        g = np.sort(perm[i * K:(i + 1) * K])
        C[np.ix_(g, g)] = _wishart(K, rng)
        pool.append(g)
    return C, np.array(pool, dtype=np.int64).reshape(n, K)


def big_index_case(K):
    """(C, groups): a Wishart covariance of 300 models and groups of K models whose indices reach 299; one group lies wholly
    beyond 255, one straddles, one is arange(K)"""
    rng = np.random.RandomState(300 + K)
    A = rng.randn(BIG_N, 4 * BIG_N)
    C = A @ A.T / (4 * BIG_N)
    hi = np.sort(np.concatenate([[BIG_N - 1], rng.choice(np.arange(256, BIG_N - 1), K - 1, replace=False)]))
    mid = np.sort(np.concatenate([[BIG_N - 1, 0], rng.choice(np.arange(1, BIG_N - 1), K - 2, replace=False)])) if K >= 2 else hi
    return C, np.array([hi, mid, np.arange(K), np.sort(rng.choice(BIG_N, K, replace=False))], dtype=np.int64)


# ---- records ------------------------------------------------------------------------------------------------------------------

RECORD_NS = (1, 2, 5, 33, 54, 55, 64)        # dynamic LDS of k_pinv_from_record crosses 48 KiB between N = 54 and 55
N_OUT, N_CAND = 3, 2
# kind -> smallest N that admits it
RECORD_KINDS = collections.OrderedDict([
    ("regular", 1), ("def1", 2), ("def2", 3), ("defhalf", 4), ("null_unsampled", 5), ("no_model0", 2), ("no_model0_singular", 5),
    ("two_pass_singular", 5), ("asym", 2), ("big0", 1), ("allzero", 1), ("regular_delta", 2), ("one_pass_delta", 2), ("no_model0_delta", 2), ("spd_delta", 1)])
DELTA = 1e-3
# the three launches of every N, six (candidate, output) slots each; a kind that N does not admit gives way to "regular"
LAUNCHES = collections.OrderedDict([
    ("A", (0.0, ("regular", "def1", "def2", "defhalf", "null_unsampled", "no_model0"))),
    ("B", (0.0, ("no_model0_singular", "asym", "big0", "allzero", "regular", "def1"))),
    ("C", (DELTA, ("two_pass_singular", "regular_delta", "big0", "one_pass_delta", "no_model0_delta", "two_pass_singular")))])


def _gram(n, rank, rng):
    """an exactly singular symmetric float64 matrix of the given rank: B B^T / 8 with small integer B (every product and sum is
    exact), so that the null space is that of the matrix in memory and not of a rounded one"""
    while True:
        B = rng.randint(-3, 4, (n, rank)).astype(np.float64)
        if np.linalg.matrix_rank(B) == rank:
            return B @ B.T / 8.0


def _spd(n, rng):
    return _spectrum(n, np.logspace(0, -2, n) if n > 1 else np.ones(1), rng) * float(rng.uniform(0.5, 4.0))


def record(kind, N, slot, delta):
    """(Phi, s1, s2, big, delta) of one record row; delta is that of the row's launch"""
    assert N >= RECORD_KINDS[kind], (kind, N)
    rng = np.random.RandomState(1009 * list(RECORD_KINDS).index(kind) + 17 * N + slot)
    ones = np.ones(N)
    junk = lambda: 5.0 * rng.randn(N, N)          # noqa: E731
    if kind == "regular":
        return _spd(N, rng), ones, ones, 1.0, delta
    if kind in ("def1", "def2", "defhalf"):
        rank = {"def1": N - 1, "def2": N - 2, "defhalf": N - N // 2}[kind]
        return _gram(N, rank, rng), ones, ones, 1.0, delta
    if kind == "null_unsampled":                  # s2 = about 3/4 of the models, s1 = s2 less one, Phi[s2, s2] of rank |s1| - 2
        s2 = np.zeros(N)
        s2[np.concatenate([[0], 1 + rng.choice(N - 1, max(3, (3 * N) // 4 - 1), replace=False)])] = 1.0
        s1 = s2.copy()
        s1[np.flatnonzero(s2)[-1]] = 0.0
        Phi = junk()                              # the rows of unsampled models are noise that must be ignored
        idx = np.flatnonzero(s2)
        Phi[np.ix_(idx, idx)] = _gram(len(idx), max(1, len(idx) - 3), rng)
        return Phi, s1, s2, 1.0, delta
    if kind in ("no_model0", "no_model0_delta"):  # model 0 (and another, where there is one) unsampled: t = the first sampled
        s = ones.copy()
        s[0] = 0.0
        if N > 3:
            s[2] = 0.0
        if kind == "no_model0_delta":             # delta != 0: mask2 is every model, so the whole matrix counts
            return _spd(N, rng), s, s, 1.0, delta
        Phi = junk()
        idx = np.flatnonzero(s)
        Phi[np.ix_(idx, idx)] = _spd(len(idx), rng)
        return Phi, s, s, 1.0, delta
    if kind == "no_model0_singular":              # s1 lacks models 0 and 1, s2 holds model 0: two passes, singular in both
        s2 = ones.copy()
        s2[1] = 0.0
        s1 = s2.copy()
        s1[0] = 0.0
        Phi = junk()
        idx = np.flatnonzero(s2)
        Phi[np.ix_(idx, idx)] = _gram(len(idx), len(idx) - 2, rng)
        return Phi, s1, s2, 1.0, delta
    if kind == "two_pass_singular":               # delta != 0 and s1 != every model: pass 1 on s1, pass 2 on all N
        s1 = ones.copy()
        s1[rng.choice(np.arange(1, N), 2, replace=False)] = 0.0
        return _gram(N, N - 2, rng), s1, s1, 1.0, delta
    if kind == "asym":
        return _spd(N, rng) + 1e-3 * rng.randn(N, N), ones, ones, 1.0, delta
    if kind == "big0":
        return _spd(N, rng), ones, ones, 0.0, delta
    if kind == "allzero":
        return _spd(N, rng), 0 * ones, 0 * ones, 1.0, delta
    if kind == "regular_delta":
        s1 = ones.copy()
        s1[N - 1] = 0.0
        return _spd(N, rng), s1, ones, 1.0, delta
    if kind == "spd_delta":
        return _spd(N, rng), ones, ones, 1.0, delta
    if kind == "one_pass_delta":                  # delta != 0 with every model in s1: one pass, singular Phi made regular by delta
        return _gram(N, N - 1, rng), ones, ones, 1.0, delta
    raise ValueError(kind)


def launch_kinds(N, launch):
    """the six kinds of one launch at this N ("regular" or "spd_delta" where N does not admit the kind)"""
    delta, kinds = LAUNCHES[launch]
    fill = "regular" if delta == 0.0 else "spd_delta"
    return [k if N >= RECORD_KINDS[k] else fill for k in kinds]


def record_rows():
    rows = []
    for N in RECORD_NS:
        for launch, (delta, _) in LAUNCHES.items():
            for slot, kind in enumerate(launch_kinds(N, launch)):
                rows.append(RecordRow("%s_N%d_%s%d" % (kind, N, launch, slot), kind, N, functools.partial(record, kind, N, slot, delta)))
    return rows


RECORD_ROWS = record_rows()
N_RECORD_ROWS = len(RECORD_NS) * len(LAUNCHES) * N_OUT * N_CAND


def launch_rows(N, launch):
    return [r for r in RECORD_ROWS if r.N == N and r.name.rsplit("_", 1)[1].startswith(launch)]


@functools.lru_cache(maxsize=None)
def record_reference(name):
    """dict of one record row: rec (float64 record), delta, V, v, status (pinv_ref.record_pinv), tolV, tolv"""
    row = next(r for r in RECORD_ROWS if r.name == name)
    Phi, s1, s2, big, delta = row.build()
    rec = ref.make_record(Phi, s1, s2, big)
    out = ref.record_pinv(rec, row.N, delta)
    out.update(rec=rec, delta=delta)
    if out["w"]:
        out["tolV"] = C_BOUND * ref.cond_kept(out["w"][0]) * ref.EPS
        out["tolv"] = C_BOUND * ref.cond_kept(out["w"][-1]) * ref.EPS
    return out

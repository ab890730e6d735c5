"""
The case table of the bluest_cov_project ABI tests (test_gpu_covproj_abi.py), generated from seeds; test_covproj_ref.py
checks on the CPU that every decision of the reference on every row is safe and that the table reaches every path.

A row: name, group ("clip" / "spg" / "budget"), C, mask, params (over oracle.covproj_ref.default_params), and for the SPG
rows K, the number of iterations compared in lock-step.
"""
import functools

import numpy as np

from oracle import covproj_ref as ref

CLIP_SIZES = (1, 2, 3, 5, 31, 32, 33, 63, 64)
SPG_SIZES = (2, 3, 6, 7, 12, 13)

# paths that no input reaches, with the reason (test_covproj_ref.py asserts that they stay unreached: a row that reaches
# one disproves the reason)
UNREACHED = {
    "lmbda:sdoty<=0": "W = mask^2 >= 0 and am() is monotone in v, so every product s_i y_i is >= 0 in float64 too: sdoty <= 0 "
                      "needs every product to be exactly zero, a step that moves no weighted entry, and such a step has "
                      "g.d = 0 and comes only from a point where gpmax is zero on the weighted entries",
    "ls:safeguard_hi": "alpha_t > 0.9 alpha means fnew < f - 0.44 alpha |g.d|, a rejected trial means fnew > fmax - 1e-4 alpha "
                       "|g.d|, and fmax >= f because the ring always holds the current f: both cannot hold with g.d <= 0",
    "status:noeig": "needs a sweep budget that fails: not to be provoked",
}

# What the table reaches but cannot judge.  Three changes of the kernel leave every compared value inside its bound and every
# branch as it is; each was built into a library and run once, and every test passed:
#   - the 1e-15 threshold applied to |m| instead of m^2 (path mask:thresholds_differ).  The only masks between the two are
#     1e-14 <= |m| < 3.2e-8, whose weight m^2 is below 1e-15: with weight 1e-16 instead of 0, x moves by about 5e-17 on the
#     weighted rows, where the one-step bound is about 3e-12.  The ratio does not depend on the scale of C, since the bound
#     grows with ||x|| as the entry's pull does, so no input separates the two thresholds through this interface.
#   - sigma_max = 0.5.  alpha_t > 0.5 alpha needs f_new < f, a rejected trial f_new > f - 1e-4 alpha |g.d|: in that sliver
#     alpha_t lies within 5e-5 alpha of the alpha / 2 that replaces it.
#   - sdoty <= 0 giving lmbda_min: the branch is unreachable (above).
# ls:gamma_decides and ls:oldest_decides exist for the same reason: an Armijo test that falls the same way under
# gamma = 1e-3, or with the ring written one slot further on, cannot see either, so the table must hold one that does not.

REQUIRED = ["clip", "clip:lower_only", "spg:odd_M", "spg:even_M", "ls:first_trial", "ls:quadratic", "ls:safeguard_lo", "ls:halve",
            "ls:nonmonotone", "ls:gamma_decides", "ls:oldest_decides", "lmbda:clamped_min", "lmbda:clamped_max", "lmbda:bb", "lmbda:start", "status:ok", "status:maxit",
            "status:maxfev", "status:nonfinite", "exit:maxfev_linesearch", "exit:maxfev_loop", "mask:thresholds_differ"]


def _spectrum(M, l, seed):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(M, M))
    C = Q @ np.diag(l) @ Q.T
    return (C + C.T) / 2


def indefinite(M, seed, nneg=2, neg=0.3):
    rng = np.random.RandomState(seed + 100)
    l = rng.uniform(0.2, 2.0, M)
    l[:min(nneg, M)] = -neg * rng.uniform(0.5, 1.0, min(nneg, M))
    return _spectrum(M, l, seed)


def mask01(M, seed, frac):
    """symmetric 0/1 mask, diagonal known, at least one unknown pair"""
    rng = np.random.RandomState(seed + 5000)
    m = np.ones((M, M))
    for i in range(M):
        for j in range(i + 1, M):
            if rng.rand() < frac:
                m[i, j] = m[j, i] = 0.0
    if m.all():
        m[0, M - 1] = m[M - 1, 0] = 0.0
    return m


def weighted_mask(M, seed):
    """0/1 mask whose known off-diagonal entries take the weights 0.5, 2, -1, 1e-8 in turn (1e-8: known, weighs nothing)"""
    m = mask01(M, seed, 0.25)
    vals, k = (0.5, 2.0, -1.0, 1.0e-8, 1.0), 0
    for i in range(M):
        for j in range(i + 1, M):
            if m[i, j] != 0.0:
                m[i, j] = m[j, i] = vals[k % len(vals)]
                k += 1
    return m


def _clip_input(kind, M, seed):
    rng = np.random.RandomState(seed)
    thr = 5.0e-14
    if kind == "indefinite":
        C = indefinite(M, seed, nneg=max(1, M // 3))
    elif kind == "spd":
        C = _spectrum(M, rng.uniform(0.5, 2.0, M), seed)
    elif kind == "negdef":
        C = _spectrum(M, -rng.uniform(0.5, 2.0, M), seed)
    elif kind == "diagonal":
        C = np.diag(rng.uniform(-1.0, 1.0, M))
    elif kind == "clustered":                          # a fourfold and an eightfold eigenvalue, none within 1e-6 of thr
        l = rng.uniform(0.3, 2.0, M)
        l[:4], l[4:12] = -0.25, 0.75
        C = _spectrum(M, l, seed)
    elif kind in ("thr0", "thr0.5"):
        C, thr = indefinite(M, seed, nneg=max(1, M // 3)), (0.0 if kind == "thr0" else 0.5)
    elif kind in ("scale_up", "scale_down"):
        C = indefinite(M, seed, nneg=max(1, M // 3)) * 2.0 ** (200 if kind == "scale_up" else -200)
    elif kind == "asymmetric":                         # the strict upper triangle is noise: eigh reads the lower one
        C = indefinite(M, seed, nneg=max(1, M // 3))
        C[np.triu_indices(M, 1)] = rng.randn(M * (M - 1) // 2)
    else:
        raise KeyError(kind)
    return C, thr


_ALL = ("indefinite", "spd", "negdef", "diagonal", "thr0", "thr0.5", "scale_up", "scale_down", "asymmetric")
CLIP_KINDS = {1: _ALL[:-1], 2: _ALL, 3: _ALL, 5: _ALL,
              31: ("indefinite", "clustered", "asymmetric", "spd", "thr0.5", "scale_up"),
              32: ("indefinite", "clustered", "asymmetric", "negdef", "thr0", "scale_down"),
              33: ("indefinite", "clustered", "asymmetric", "diagonal"),
              63: ("indefinite", "clustered", "asymmetric"),
              64: ("indefinite", "clustered", "asymmetric")}


def _row(name, group, C, mask, K=None, **params):
    return {"name": name, "group": group, "C": C, "mask": mask, "params": params, "K": K}


def overflow_case():
    """M = 4, entries near 1e155: sum a^2 overflows float64, the matrix itself is far from it"""
    return _row("overflow_M4", "overflow", indefinite(4, 404) * 1.0e155, np.ones((4, 4)))


@functools.lru_cache(maxsize=None)
def all_cases():
    rows = []
    for M in CLIP_SIZES:
        for k, kind in enumerate(CLIP_KINDS[M]):
            C, thr = _clip_input(kind, M, 1000 * M + k)
            rows.append(_row("clip_%s_M%d" % (kind, M), "clip", C, np.ones((M, M)), spd_threshold=thr))
    # a mask that is nonzero everywhere but not 1: still the single clip
    rows.append(_row("clip_weights_M5", "clip", indefinite(5, 55), np.where(np.eye(5) > 0, 1.0, -2.0)))
    # ---- SPG, lock-step ------------------------------------------------------------------------------------------------
    spg = functools.partial(_row, group="spg")
    rows += [
        spg("spg_10pc_M12_h10", C=indefinite(12, 12), mask=mask01(12, 12, 0.1), K=6),
        spg("spg_40pc_M13_h10", C=indefinite(13, 13), mask=mask01(13, 13, 0.4), K=6),
        spg("spg_40pc_M6_h1", C=indefinite(6, 6), mask=mask01(6, 6, 0.4), K=8, hlength=1),
        spg("spg_40pc_M6_h2", C=indefinite(6, 6), mask=mask01(6, 6, 0.4), K=8, hlength=2),
        spg("spg_10pc_M7_h64", C=indefinite(7, 7), mask=mask01(7, 7, 0.1), K=8, hlength=64),
        # M = 2 with a pair known at weight 0.5 and one variance unknown (any mask is the caller's right)
        spg("spg_unknown_variance_M2", C=np.array([[1.0, 3.0], [3.0, 0.0]]), mask=np.array([[1.0, 0.5], [0.5, 0.0]]), K=8, eps=1e-7),
        spg("spg_40pc_M3", C=indefinite(3, 3, nneg=1), mask=mask01(3, 3, 0.4), K=8, eps=1e-7),
        # the same input under two history lengths: hlength = 10 accepts a step with f_new > f that hlength = 1 rejects
        spg("spg_nonmonotone_M7_h10", C=indefinite(7, 32), mask=mask01(7, 32, 0.4), K=4, hlength=10),
        spg("spg_nonmonotone_M7_h1", C=indefinite(7, 32), mask=mask01(7, 32, 0.4), K=4, hlength=1),
        # and under hlength = 2, where that step is iteration 2: the ring is {f0, f1}, f1 < f2 < f0, so the step is accepted
        # only because f0 is still in the window.  A ring written one slot further on differs from the kernel's in one
        # iteration only, number hlength, where it has already lost f0 (afterwards both hold the last hlength values), and
        # hlength = 2 is the window where that iteration can be reached and judged in a few steps.
        spg("spg_nonmonotone_M7_h2", C=indefinite(7, 32), mask=mask01(7, 32, 0.4), K=4, hlength=2),
    ]
    # lmbda_min = lmbda_max: the first trial overshoots more and more
    for M, lam in ((6, 8.0), (7, 4.0), (6, 30.0), (7, 300.0), (12, 3000.0), (13, 30.0)):
        rows.append(spg("spg_fixed_lmbda%g_M%d" % (lam, M), C=indefinite(M, 10 + M), mask=mask01(M, M, 0.4), K=3 if M > 7 else 4,
                        lmbda_min=lam, lmbda_max=lam))
    # a step length at which the first trial of iteration 1 gains (f_new - f) / (g.d) = 4.9e-4 of the predicted decrease:
    # accepted with gamma = 1e-4, by a margin of 3.9e-4 |g.d|, and rejected by any gamma above 4.9e-4 (lambda from a
    # bisection on the reference: the ratio falls by about 0.1 per unit of lambda there, so three decimals place it)
    rows.append(spg("spg_gamma_window_M6", C=indefinite(6, 16), mask=mask01(6, 6, 0.4), K=3, lmbda_min=16.26, lmbda_max=16.26))
    rows += [
        # converges inside K: the last call must report OK with the reference's it and count
        spg("spg_converges_M6", C=indefinite(6, 64), mask=mask01(6, 64, 0.4), K=8, eps=1e-2),
        spg("spg_weights_M7", C=indefinite(7, 77), mask=weighted_mask(7, 77), K=6),
        spg("spg_weights_M12", C=indefinite(12, 122), mask=weighted_mask(12, 122), K=5),
        spg("spg_weights_M3", C=indefinite(3, 33, nneg=1), mask=np.array([[1.0, 1e-8, 0.0], [1e-8, 1.0, -1.0], [0.0, -1.0, 2.0]]),
            K=8, eps=1e-7),
    ]
    return tuple(rows)


def by_group(group):
    return [r for r in all_cases() if r["group"] == group]


def case(name):
    return next(r for r in all_cases() if r["name"] == name)


def _poke(A, i, j, v):
    A = A.copy()
    A[i, j] = v
    return A


def budget_cases():
    """(row, expected info, expected it or None, expected count or None, which exit)"""
    base = case("spg_fixed_lmbda30_M6")
    free = case("spg_40pc_M6_h2")

    def with_(r, name, C=None, mask=None, **p):
        return dict(r, name=name, group="budget", C=r["C"] if C is None else C, mask=r["mask"] if mask is None else mask,
                    params=dict(r["params"], **p))
    return [
        (with_(free, "maxit0", maxit=0), ref.MAXIT, 0, 1, None),
        (with_(free, "maxfev0", max_fevals=0), ref.MAXFEV, 0, 1, "exit:maxfev_loop"),
        (with_(free, "maxfev1", max_fevals=1), ref.MAXFEV, 0, 1, "exit:maxfev_loop"),
        (with_(base, "maxfev2_overshoot", max_fevals=2), ref.MAXFEV, 1, 2, "exit:maxfev_linesearch"),
        (with_(free, "maxfev_between", max_fevals=8), ref.MAXFEV, 2, 8, "exit:maxfev_loop"),
        (with_(free, "eps_large", eps=10.0), ref.OK, 0, 1, None),
        (with_(free, "nan_under_zero_mask", C=np.where(free["mask"] == 0.0, np.nan, free["C"]), maxit=2), ref.MAXIT, 2, None, None),
        (with_(free, "nan_known", C=_poke(free["C"], 1, 1, np.nan)), ref.NONFINITE, 0, 0, None),
        (with_(free, "inf_known", C=_poke(free["C"], 2, 2, np.inf)), ref.NONFINITE, 0, 0, None),
        (with_(free, "nan_in_mask", mask=_poke(free["mask"], 0, 1, np.nan)), ref.NONFINITE, 0, 0, None),
        (with_(free, "inf_in_mask", mask=_poke(free["mask"], 3, 3, -np.inf)), ref.NONFINITE, 0, 0, None),
    ]


MULTI_PARAMS = {"eps": 1e-2, "maxit": 5, "max_fevals": 9}


def multi_case():
    """five outputs of one launch (M = 6, shared parameters) that end in five different states: [(name, C, mask, info)]"""
    ones = np.ones((6, 6))
    return [("clip", indefinite(6, 90), ones, ref.OK),
            ("spg_ok", indefinite(6, 64), mask01(6, 64, 0.4), ref.OK),
            ("spg_maxit", indefinite(6, 60), mask01(6, 60, 0.4), ref.MAXIT),
            ("spg_maxfev", indefinite(6, 77, neg=0.05), mask01(6, 77, 0.4), ref.MAXFEV),
            ("nonfinite", _poke(indefinite(6, 64), 1, 1, np.nan), mask01(6, 64, 0.4), ref.NONFINITE)]


@functools.lru_cache(maxsize=None)
def reference(name):
    """the reference's run of a row, once per process: the first K iterations of an SPG row, everything of the others"""
    for r in all_cases() + tuple(b[0] for b in budget_cases()) + (overflow_case(),):
        if r["name"] == name:
            return ref.run_ld(r["C"], r["mask"], r["params"], max_steps=r["K"] if r["group"] == "spg" else None)
    raise KeyError(name)


# ---- the recorded runs of the reference project (tests/golden/covproj_*_M*.npz) -------------------------------------------
# The recorded run of this input (one matrix, two fixtures) takes 225 iterations, the restatement 221: at iteration 88 an
# Armijo test is decided by 7.6e-8 where rounding in the projections can move it by 1.4e-7, and 20 more tests like it follow.
# Such a run is not determined by its input in float64; these two are judged on err (and cov) alone.
FIXTURE_MARGINAL = {"bypass_M7", "early_return_M7"}


def fixture_inputs(g, n):
    """(C, mask, params) as BLUEProblem.project_covariance hands output n of a fixture to the kernel"""
    C = g["C"][n]
    mask = (~np.isinf(C)).astype(np.float64)
    if int(g["call"]) == 0 and bool(g["remove_uncorrelated"]):
        mask[C == 0] = 0.0
    np.fill_diagonal(mask, 1.0)
    params = {"maxit": int(g["maxit"])} if int(g["maxit"]) >= 0 else {}
    return np.where(mask > 0, C, 0.0), mask, params


# ---- the rows whose results are held bit for bit (tests/golden/covproj_bits_parent.npz, test_gpu_covproj_bits.py) --------
# The smallest that reach each part of the shared eigensolver: one pair and one step per sweep (M = 2); an odd size, so the
# pad index is live (M = 3); M = 4, plain and with entries whose squares overflow; 16 rotations per step with and without
# the pad (M = 31, 32); more 2 x 2 blocks per step (528) than the workgroup has threads (M = 64); and three SPG iterations,
# so that projections chain.
BITS_FIELDS = ("X", "f", "gpmax", "it", "count", "info")


@functools.lru_cache(maxsize=None)
def bits_cases():
    return (case("clip_indefinite_M2"), case("clip_indefinite_M3"),
            _row("clip_indefinite_M4", "clip", indefinite(4, 4000), np.ones((4, 4)), spd_threshold=5.0e-14), overflow_case(),
            case("clip_indefinite_M31"), case("clip_clustered_M32"), case("clip_indefinite_M64"),
            dict(case("spg_40pc_M13_h10"), name="spg_40pc_M13_h10_maxit3", params={"maxit": 3}))


BITS_NAMES = tuple(r["name"] for r in bits_cases())


def bits_record(solo, row):
    """what the record holds of one row: the six outputs of one call (`solo(row)`: one launch, one output), keyed <name>/<field>"""
    X, f, gpmax, it, count, info = solo(row)
    vals = (X, np.float64(f), np.float64(gpmax), np.int64(it), np.int64(count), np.int32(info))
    return {"%s/%s" % (row["name"], k): np.asarray(v) for k, v in zip(BITS_FIELDS, vals)}

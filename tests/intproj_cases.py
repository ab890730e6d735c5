"""
The inputs of the integer-projection kernel tests at the kernel's interface (bluest_intproj_eval, csrc/intproj.hip), with their
80-bit reference, shared by the CPU tests (test_intproj_ref.py: the reference is sound, the table reaches every instantiation
k_intproj<NT> with and without pads) and the GPU tests (test_gpu_intproj.py: the kernel equals the reference).  numpy only.

One LAUNCH is what the kernel takes, in float64: base (n_out, N*N), cols (n_out, LL, N*N), ms (n_c, LL); candidate c of output
o is Phi = base[o] + sum_j ms[c, j] cols[o, j], V = (Phi[sup, sup])^-1 [0, 0] on sup = {a: Phi_aa > 0}, +inf when model 0 is
not in sup or Phi[sup, sup] is not positive definite.  The same float64 arrays go to the kernel and to the reference, so only
the kernel's arithmetic is measured.

Built as the library builds them (integer._search): C_o = synth.wishart_covariance(N, o), base = sum_g m_g scatter(inv(C_o[g,
g])) over the singletons and about 3N random groups of 2-3 models with integer allocations 1..8, the LL columns the scattered
inverses of free groups of 1..4 models; with n_out > 1 some (output, free group) pairs keep an all-zero column (the output
does not have the group: `in_out` of integer._search).  Each float64 group inverse is symmetrised, (B + B^T) / 2, so that base and
columns are symmetric bit for bit: the elimination of csrc/solve.hpp reads a pivot row's entry (j, c) as entry (c, j), and what an
asymmetry of the inputs would do to V is not the kernel's arithmetic.

A launch shares its base among its candidates, and a model that a candidate does not support must have rows and columns that
are exactly zero in base and in every column (never reached by cancelling ms against base).  So the support patterns are
launches of their own -- VARIANTS: per (N, LL, n_out) one launch each for
    full    every model in base; candidates: dense (ms in 0..5, twice), all zero, indefinite, non-integer with one entry LARGE
    sparse  models N-1, N//2 and 1 in no group at all (N >= 4); dense, all zero, non-integer / large
    nom0    model 0 in no group at all; dense, all zero: +inf (with N = 1 nothing is supported at all)
    ill     every group with model N-1, fixed or free, WEAK = 1e-7 times weaker (cond 1e7 .. 1e9; with 1e-5 this construction
            gives 1e5 .. 1e6, on both sides of the threshold of the cap; at N = 2, where model 0 meets the weak model in every
            pair, 1e-9 for the same range); dense, all zero (N >= 2)
The indefinite candidate (N >= 2) takes a negative multiple t of free group 0: every diagonal entry stays positive (t below
min_a B_aa / P_aa) while Phi has a negative eigenvalue (t above 1 / lambda_max(B^-1 P)); the builder asserts that every (candidate,
output) is either positive definite with cond <= 1e10, or has a smallest eigenvalue below -1e-6 times its largest entry; that
margin is far beyond what float64 rounding moves an eigenvalue by (N eps |Phi|), so the reference takes the decision from the
float64 eigenvalues and V from ld_eval.solve_ld.  A finite candidate is either well-conditioned (cond <= 1e6, and then its
derived bound must lie below the cap) or ill-conditioned on purpose (1e6 < cond <= 1e10): LARGE = 1e9 on one entry puts the
candidates whose large group does not cover every model into the second class (1e6 would leave them at cond 1e3 .. 1e6, where
the cap is tighter than float64 arithmetic can promise).  With 16 outputs (N = 64) only the `full` launch runs: the extra
outputs are about addressing, not about support patterns.

Tolerance of V (as _bounds of test_gpu_launch_matrix.py; the kernel forms an entry with an fma chain over the base entry and LL
products, 1 + LL terms):
    phi_rel = (1 + LL) eps max_ab (|base_ab| + sum_j |ms_j cols_j,ab|) / max |Phi|
    tol_V   = 2 cond(Phi[sup, sup]) (phi_rel + N eps), capped at 1e-11 (the parity tests' bar for stored inverses) when
              cond <= 1e6; the ill-conditioned candidates are held to the derived bound itself.
"""
import numpy as np

from bluest_amd import synth
from oracle import ld_eval

LD = np.longdouble
EPS = ld_eval.EPS
CAP, COND_WELL, COND_MAX, INDEF_MARGIN = 1e-11, 1e6, 1e10, 1e-6
WEAK, WEAK_N2, LARGE = 1e-7, 1e-9, 1e9
LLS = (1, 7, 32)
VARIANTS = ("full", "sparse", "nom0", "ill")
OK, NOM0, SING = "ok", "no_model0", "singular"


def nt_values():
    """the instantiations k_intproj<NT> the library is built with (host only)"""
    from bluest_amd.plan import launch_sets
    return sorted(launch_sets()["nt"])


def nt_of(N, nts):
    return next(nt for nt in nts if N <= nt)


def table_n(nts=None):
    """per NT: N = NT (no pads, clear_pads is skipped) and N = previous NT + 1 (the most pads); and N = 2"""
    nts = nt_values() if nts is None else sorted(nts)
    out, prev = {2}, 0
    for nt in nts:
        out |= {nt, prev + 1}
        prev = nt
    return sorted(out)


def settings(N, nts=None):
    """(LL, n_out) of the launches of one N"""
    nts = nt_values() if nts is None else nts
    outs = (1, 3, 16) if N == max(nts) else (1, 3)
    return [(LL, n_out) for LL in LLS for n_out in outs]


def absent_models(N, variant):
    """models in no group of the launch (rows and columns exactly zero everywhere); None: the variant does not exist at this N"""
    if variant == "sparse":
        return sorted({N - 1, N // 2, 1}) if N >= 4 else None
    if variant == "nom0":
        return [0]
    if variant == "ill":
        return [] if N >= 2 else None
    return []


def _scatter(N, C, g, weight=1.0):
    out = np.zeros((N, N))
    if len(g):
        B = np.linalg.inv(C[np.ix_(g, g)])
        out[np.ix_(g, g)] = weight * (0.5 * (B + B.T))
    return out


def judge(N, base_o, cols_o, ms_c):
    """one (candidate, output): Phi in longdouble, and the float64 judgement of the module docstring --
    dict(kind, cond, derived, sup, A): kind OK / NOM0 / SING, or 'unclear' for a candidate that the table must not contain"""
    LL = len(ms_c)
    phi = np.asarray(base_o, dtype=LD).copy()
    mag = np.abs(phi)
    for j in range(LL):
        t = LD(ms_c[j]) * np.asarray(cols_o[j], dtype=LD)
        phi += t
        mag += np.abs(t)
    phi = phi.reshape(N, N)
    d = np.diag(phi)
    sup = np.flatnonzero(d > 0)
    out = dict(kind="unclear", cond=np.inf, derived=np.inf, sup=sup, A=None)
    off = np.flatnonzero(~(d > 0))
    if (d < 0).any() or mag.reshape(N, N)[off].any() or mag.reshape(N, N)[:, off].any():
        return out                                  # a model may only be unsupported with exact zeros, never by cancellation
    if len(sup) == 0 or sup[0] != 0:
        out.update(kind=NOM0, cond=1.0)
        return out
    A = phi[np.ix_(sup, sup)]
    out["A"] = A
    A64 = A.astype(np.float64)
    ev = np.linalg.eigvalsh(A64)
    if ev[0] < -INDEF_MARGIN * np.abs(A64).max():
        out["kind"] = SING
        return out
    if not ev[0] > 0:
        return out
    cond = float(ev[-1] / ev[0])                    # 2-norm condition of a symmetric positive definite matrix
    phi_rel = float((1 + LL) * EPS * mag.max() / np.abs(phi).max())
    derived = 2.0 * cond * (phi_rel + N * EPS)
    out.update(cond=cond, derived=derived)
    if cond <= COND_MAX and (cond > COND_WELL or derived <= CAP):
        out["kind"] = OK
    return out


def _indefinite_ms(L, rng):
    """ms = (-t, small integers ...): see the module docstring; t from the first fraction of the window that leaves every output
    clearly positive definite or clearly indefinite, and at least one indefinite"""
    N, LL, n_out = L["N"], L["LL"], L["n_out"]
    rest = np.concatenate([[0.0], rng.randint(0, 3, LL - 1).astype(np.float64)])
    lo, hi = np.inf, np.inf
    for o in range(n_out):
        P = L["cols"][o, 0].reshape(N, N)
        if not P.any():
            continue
        B = (L["base"][o] + rest @ L["cols"][o]).reshape(N, N)
        dp = np.diag(P) > 0
        hi = min(hi, float((np.diag(B)[dp] / np.diag(P)[dp]).min()))
        Li = np.linalg.inv(np.linalg.cholesky(B))
        lo = min(lo, 1.0 / float(np.linalg.eigvalsh(Li @ P @ Li.T)[-1]))
    assert lo < hi, (N, LL, n_out, lo, hi)
    for frac in (0.5, 0.7, 0.3, 0.85, 0.15, 0.93, 0.6, 0.4, 0.97, 0.08):
        ms = rest.copy()
        ms[0] = -(lo + frac * (hi - lo))
        kinds = [judge(N, L["base"][o], L["cols"][o], ms)["kind"] for o in range(n_out)]
        if "unclear" not in kinds and SING in kinds:
            return ms
    raise AssertionError("no clean indefinite candidate for N=%d LL=%d n_out=%d" % (N, LL, n_out))


_LAUNCHES = {}


def launch(N, LL, n_out, variant):
    """dict(N, LL, n_out, variant, base, cols, ms, kinds, absent, free, in_out) of one launch, or None if the variant does not exist
    at N; built once per process and shared"""
    key = (N, LL, n_out, variant)
    if key not in _LAUNCHES:
        _LAUNCHES[key] = None if absent_models(N, variant) is None else _build(N, LL, n_out, variant)
    return _LAUNCHES[key]


def _build(N, LL, n_out, variant):
    absent = absent_models(N, variant)
    weak_scale = WEAK if N > 2 else WEAK_N2
    rng = np.random.RandomState(100003 * VARIANTS.index(variant) + 1000 * N + 10 * LL + n_out)
    live = np.array([a for a in range(N) if a not in absent], dtype=np.int64)
    weak = N - 1 if variant == "ill" else -1

    def pick(kmax):
        k = rng.randint(1, kmax + 1) if kmax >= 1 else 0
        return np.sort(rng.choice(live, k, replace=False)) if k else np.zeros(0, dtype=np.int64)

    fixed = [np.array([a]) for a in live]
    if len(live) >= 2:
        fixed += [np.sort(rng.choice(live, min(rng.randint(2, 4), len(live)), replace=False)) for _ in range(3 * N)]
    alloc = rng.randint(1, 9, len(fixed)).astype(np.float64)
    free = [pick(min(4, len(live))) for _ in range(LL)]
    scale = np.array([weak_scale if weak in g else 1.0 for g in free])
    in_out = np.ones((n_out, LL), dtype=bool)
    if n_out > 1:
        in_out[1:] = rng.rand(n_out - 1, LL) > 0.3
        in_out[n_out - 1, LL - 1] = False
    base = np.zeros((n_out, N * N))
    cols = np.zeros((n_out, LL, N * N))
    for o in range(n_out):
        C = synth.wishart_covariance(N, o)[0]
        for g, m in zip(fixed, alloc):
            base[o] += _scatter(N, C, g, m * (weak_scale if weak in g else 1.0)).ravel()
        for j, g in enumerate(free):
            if in_out[o, j]:
                cols[o, j] = _scatter(N, C, g).ravel()
    L = dict(N=N, LL=LL, n_out=n_out, variant=variant, base=base, cols=cols, absent=list(absent), free=free, in_out=in_out)
    dense = lambda: rng.randint(0, 6, LL).astype(np.float64)      # noqa: E731
    ms, kinds = [dense()], ["dense"]
    if variant == "full":
        ms.append(dense()); kinds.append("dense")
    if variant == "ill":
        ms[0] = rng.randint(1, 6, LL) * scale
    ms.append(np.zeros(LL)); kinds.append("zero")
    if variant == "full" and N >= 2:
        ms.append(_indefinite_ms(L, rng)); kinds.append("indefinite")
    if variant in ("full", "sparse"):
        big = 3.0 * rng.rand(LL)
        big[rng.randint(LL)] = LARGE
        ms.append(big); kinds.append("large")
    L["ms"], L["kinds"] = np.array(ms), kinds
    return L


def launches(N, nts=None):
    out = []
    for LL, n_out in settings(N, nts):
        for v in VARIANTS if n_out <= 3 else VARIANTS[:1]:
            L = launch(N, LL, n_out, v)
            if L is not None:
                out.append(L)
    return out


def reference_one(N, base_o, cols_o, ms_c):
    """dict(kind, V, cond, tol, derived, sup) of one (candidate, output); base_o (N*N), cols_o (LL, N*N), ms_c (LL)"""
    r = judge(N, base_o, cols_o, ms_c)
    assert r["kind"] != "unclear", (N, r["cond"], r["derived"])
    A = r.pop("A")
    if r["kind"] != OK:
        r.update(V=np.inf, tol=0.0)
        return r
    r["V"] = float(ld_eval.solve_ld(A, np.eye(len(r["sup"]), 1, dtype=LD).ravel())[0])
    r["tol"] = min(CAP, r["derived"]) if r["cond"] <= COND_WELL else r["derived"]
    return r


_REFS = {}


def reference(L):
    """refs[c][o] of a launch, computed once per process and shared (read only)"""
    key = (L["N"], L["LL"], L["n_out"], L["variant"])
    if key not in _REFS:
        _REFS[key] = [[reference_one(L["N"], L["base"][o], L["cols"][o], L["ms"][c]) for o in range(L["n_out"])]
                      for c in range(len(L["ms"]))]
    return _REFS[key]


def phi64(L, c, o):
    """Phi of one (candidate, output) summed in plain float64"""
    N = L["N"]
    phi = L["base"][o].copy()
    for j in range(L["LL"]):
        phi += L["ms"][c, j] * L["cols"][o, j]
    return phi.reshape(N, N)


# ---- the host search that feeds the kernel (integer._search): two problems with 2^9 .. 2^10 candidates ---------------------------
# Model costs are powers of two (synth.model_costs), so every candidate's cost is an exact dyadic sum: equal costs are equal bits
# whatever the order of the summation, and no cost comes near 1.0001 * budget by rounding.

def search_problem_single():
    """one output, N = 9, groups of up to 3 models plus a SECOND COPY of the pair (0, 1) at the end of the pairs: free entries 0 and
    9 (`tie`) have equal columns, equal costs and the bounds 0 / 1, so that candidates which swap them have the same Phi bit for
    bit (fma(0, c, x) = x).  No fixed group has model 0: the host's model-0 filter decides, and the winners of both modes take
    exactly one of the two copies.  caps: model 3 may have 11 samples in all (7 are fixed), which half of the candidates keep
    and the best points of both modes without the cap do not"""
    N = 9
    groups = synth.all_groups(N, 3)
    groups[1] = np.vstack([groups[1], [[0, 1]]])
    flat = [tuple(g) for gk in groups for g in gk.tolist()]
    ix = lambda *g: flat.index(tuple(g))      # noqa: E731
    T1, T2 = ix(0, 1), len(flat) - len(groups[2]) - 1
    assert flat[T2] == (0, 1) and T2 != T1
    sol = np.zeros(len(flat))
    for a, m in zip(range(1, 9), [2, 3, 4, 6, 8, 12, 16, 24]):
        sol[ix(a)] = m
    sol[ix(1, 2)], sol[ix(3, 5, 7)], sol[ix(4, 6)] = 2, 3, 5
    free = [(T1, 0), (ix(0, 2, 3), 0), (ix(1, 3), 1), (ix(2, 4), 2), (ix(5, 6), 1), (ix(7, 8), 3), (ix(1, 2, 4), 0), (ix(3, 6, 8), 2),
            (ix(5), 3), (T2, 0)]
    idx = np.array([f[0] for f in free], dtype=np.int64)
    lb = np.array([f[1] for f in free], dtype=np.int64)
    sol[idx] = lb + 0.5
    return dict(name="single_n9", N=N, kmax=3, n_out=1, groups=groups, multi_groups=None, w=synth.model_costs(N), sol=sol, idx=idx,
                lb=lb, ub=lb + 1, tie=(0, len(free) - 1), multi=False, budget=10.25, eps=[np.sqrt(0.0946)], caps=[(3, 11)])


def search_problem_ragged(G):
    """three outputs on subsets of 40 groups (the fixture mosap_n6_o3_ragged.npz, passed in as G): 9 free entries, four of them
    with model 0 and no fixed group with it, two outputs lack two free groups each (`in_out`).  caps on models 1 and 2 keep
    somewhat more than a quarter of the candidates and exclude the best point of the budget mode without them"""
    n, n_out, kmax = int(G["n"]), int(G["n_out"]), int(G["kmax"])
    groups = [np.asarray(G["g_k%d" % k], dtype=np.int64) for k in range(1, kmax + 1)]
    multi_groups = [[np.asarray(G["mg%d_k%d" % (o, k)], dtype=np.int64) for k in range(1, kmax + 1)] for o in range(n_out)]
    flat = [tuple(g) for gk in groups for g in gk.tolist()]
    rng = np.random.RandomState(5)
    sol = np.zeros(len(flat))
    for a, m in zip(range(1, 6), [3, 5, 7, 9, 12]):
        sol[flat.index((a,))] = m
    non0 = [i for i, g in enumerate(flat) if 0 not in g and len(g) > 1]
    with0 = [i for i, g in enumerate(flat) if 0 in g and len(g) == 3]
    fx = rng.choice(non0, 3, replace=False)
    sol[fx] = rng.randint(1, 5, 3)
    free = [0, flat.index((0, 2))] + list(rng.choice(with0, 2, replace=False)) \
        + list(rng.choice([i for i in non0 if i not in fx], 5, replace=False))
    idx = np.array(free, dtype=np.int64)
    lb = np.concatenate([[0, 0, 0, 0], rng.randint(0, 3, 5)]).astype(np.int64)
    sol[idx] = lb + 0.5
    return dict(name="ragged_n6_o3", N=n, kmax=kmax, n_out=n_out, groups=groups, multi_groups=multi_groups, w=synth.model_costs(n),
                sol=sol, idx=idx, lb=lb, ub=lb + 1, tie=None, multi=True, budget=16.7, eps=list(np.sqrt([0.196, 0.21, 0.18])),
                caps=[(1, 15), (2, 16)])


def cap_rows(P):
    """max_samples_info of integer._search for the problem's caps [(model, most samples of it)]: (ES, rhs), one indicator row
    over the global groups per capped model"""
    flat = [g for gk in P["groups"] for g in gk.tolist()]
    ES = [np.array([1 if model in g else 0 for g in flat], dtype=np.int64) for model, _ in P["caps"]]
    return ES, [float(r) for _, r in P["caps"]]


def all_candidates(P):
    """(2^LL, LL) multipliers in the order of integer._search: bit j of the code picks ub[j]"""
    LL = len(P["idx"])
    bits = (np.arange(1 << LL)[:, None] >> np.arange(LL)[None, :]) & 1
    return np.where(bits == 1, P["ub"][None, :], P["lb"][None, :]).astype(np.float64)


def reference_batch(N, base, cols, ms):
    """(V (n_c, n_out) float64, tol (n_c, n_out), largest cond) of every candidate of a launch by reference_one"""
    n_out = base.shape[0]
    V = np.full((len(ms), n_out), np.inf)
    tol = np.zeros((len(ms), n_out))
    cond = 1.0
    for c in range(len(ms)):
        for o in range(n_out):
            r = reference_one(N, base[o], cols[o], ms[c])
            V[c, o], tol[c, o] = r["V"], r["tol"]
            if r["kind"] == OK:
                cond = max(cond, r["cond"])
    return V, tol, cond

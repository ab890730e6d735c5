"""
Host-side mirror of the hot-path part of bluest/misc.py (reference lines cited per function).  Same names,
argument meaning and error behaviour; every number comes from libbluest_hip.so (no CPU fallback).

The `*_c` functions reproduce the call shapes of the reference's native module `_cmisc_bluest`
(bluest/cmisc.cpp:99-110): they accumulate into their first argument in place and return None.
"""
import numpy as np

from . import _lib
from ._lib import check, ptr


def _c(a, dtype):
    return np.ascontiguousarray(a, dtype=dtype)


def _inplace(a, name):
    if not (isinstance(a, np.ndarray) and a.dtype == np.float64 and a.flags.c_contiguous and a.flags.writeable):
        # the reference silently copies such an argument and loses the result; be loud instead
        raise TypeError("%s must be a writeable C-contiguous float64 array (it is accumulated in place)" % name)
    return a


# ---- _cmisc_bluest call shapes ---------------------------------------------------------------------------

def assemble_psi_c(psi, N, k, Lk, groupsk, invcovsk):
    """cmisc.cpp:10-23"""
    g, ic = _c(groupsk, np.int64), _c(invcovsk, np.float64)
    check(_lib.lib().bluest_assemble_psi(ptr(_inplace(psi, "psi")), int(N), int(k), int(Lk), ptr(g), ptr(ic)))


def objectiveK_c(PHI, N, k, Lk, mk, groupsk, invcovsk):
    """cmisc.cpp:25-40; mk float64 or int64 (overloads :104-105)"""
    g, ic = _c(groupsk, np.int64), _c(invcovsk, np.float64)
    mk = np.ascontiguousarray(mk)
    if np.issubdtype(mk.dtype, np.integer):
        mk = _c(mk, np.int64)
        check(_lib.lib().bluest_objectiveK_i64(ptr(_inplace(PHI, "PHI")), int(N), int(k), int(Lk), ptr(mk), ptr(g), ptr(ic)))
    else:
        mk = _c(mk, np.float64)
        check(_lib.lib().bluest_objectiveK_f64(ptr(_inplace(PHI, "PHI")), int(N), int(k), int(Lk), ptr(mk), ptr(g), ptr(ic)))


def gradK_c(grad, k, Lk, groupsk, invcovsk, invPHI_0):
    """cmisc.cpp:58-72"""
    g, ic, v = _c(groupsk, np.int64), _c(invcovsk, np.float64), _c(invPHI_0, np.float64)
    check(_lib.lib().bluest_gradK(ptr(_inplace(grad, "grad")), int(k), int(Lk), ptr(g), ptr(ic), ptr(v), len(v)))


def cleanupK_c(X, k, Lk, groupsk, invcovsk, invPHI_0):
    """cmisc.cpp:42-56 (quirk of line 51 kept)"""
    g, ic, v = _c(groupsk, np.int64), _c(invcovsk, np.float64), _c(invPHI_0, np.float64)
    check(_lib.lib().bluest_cleanupK(ptr(_inplace(X, "X")), int(k), int(Lk), ptr(g), ptr(ic), ptr(v), len(v)))


def hessKQ_c(hess, N, k, q, Lk, Lq, groupsk, groupsq, invcovsk, invcovsq, invPHI):
    """cmisc.cpp:74-97"""
    gk, gq = _c(groupsk, np.int64), _c(groupsq, np.int64)
    ick, icq, P = _c(invcovsk, np.float64), _c(invcovsq, np.float64), _c(invPHI, np.float64)
    check(_lib.lib().bluest_hessKQ(ptr(_inplace(hess, "hess")), int(N), int(k), int(q), int(Lk), int(Lq), ptr(gk), ptr(gq),
                                   ptr(ick), ptr(icq), ptr(P)))


# ---- bluest/misc.py:600-629 wrappers ---------------------------------------------------------------------

def assemble_psi(N, k, Lk, groupsk, invcovsk):
    """misc.py:600-604"""
    psi = np.zeros((N * N, Lk), order="C")
    assemble_psi_c(psi.reshape(-1), N, k, Lk, np.asarray(groupsk).ravel(order="C"), invcovsk)
    return psi


def cleanupK(k, Lk, groupsk, invcovsk, invPHI):
    """misc.py:606-610"""
    N = invPHI.shape[0]
    X = np.zeros((N, Lk), order="C")
    cleanupK_c(X.reshape(-1), k, Lk, np.asarray(groupsk).ravel(order="C"), invcovsk, invPHI[0])
    return X


def objectiveK(N, k, Lk, mk, groupsk, invcovsk):
    """misc.py:612-616 as intended (the reference wrapper forgets N and raises TypeError)"""
    PHI = np.zeros((N * N,))
    objectiveK_c(PHI, N, k, Lk, mk, np.asarray(groupsk).ravel(order="C"), invcovsk)
    return PHI


def gradK(k, Lk, groupsk, invcovsk, invPHI):
    """misc.py:618-622"""
    grad = np.zeros((Lk,))
    gradK_c(grad, k, Lk, np.asarray(groupsk).ravel(order="C"), invcovsk, invPHI[0])
    return grad


def hessKQ(k, q, Lk, Lq, groupsk, groupsq, invcovsk, invcovsq, invPHI):
    """misc.py:624-629"""
    N = invPHI.shape[0]
    hess = np.zeros((Lk, Lq), order="C")
    hessKQ_c(hess.reshape(-1), N, k, q, Lk, Lq, np.asarray(groupsk).ravel(order="C"), np.asarray(groupsq).ravel(order="C"),
             invcovsk, invcovsq, np.asarray(invPHI).ravel(order="C"))
    return hess


def group_pinv(C, k, groupsk):
    """sap.py:69-79 for one group size: flat (Lk*k*k) pseudo-inverses of C[g,g], computed on the GPU"""
    C = _c(C, np.float64)
    g = _c(np.asarray(groupsk).ravel(order="C"), np.int64)
    Lk = len(g) // k
    out = np.empty(Lk * k * k, dtype=np.float64)
    check(_lib.lib().bluest_group_pinv(ptr(C), C.shape[0], int(k), int(Lk), ptr(g), ptr(out)))
    return out


def get_nnz_rows_cols(m, groups, cumsizes):
    """misc.py:453-457 (host index bookkeeping, used by PHIinvY0-style callers; the GPU path carries the same
    information as the per-model indicators of the Phi record)"""
    K = len(cumsizes) - 1
    ms = [m[cumsizes[k]:cumsizes[k + 1]] for k in range(K)]
    out = np.unique(np.concatenate([groups[k][abs(ms[k]) > 1.0e-6].flatten() for k in range(K)]))
    return out.reshape((len(out), 1)), out.reshape((1, len(out)))


# ---- MFMC (bluest/misc.py:48-130, 141-175, 384-449): numpy mirrors for ONE model subset -------------------------------
# O(L) each (the brute-force rounding O(2^L)); the search over subsets is bluest_mfmc_search (csrc/mfmc.hip).  Ties of |rho| and
# of the allocation are ordered as a stable sort orders them (the reference's np.argsort is not stable on every machine).

def mfmc_order(rhos):
    """np.argsort(abs(rhos))[::-1] with ties by decreasing position (misc.py:57, 90)"""
    idx = np.argsort(np.abs(rhos), kind="stable")[::-1]
    assert idx[0] == 0
    return idx


def mfmc_integer_bounds(sol):
    """get_feasible_integer_bounds(sol, len(sol)) of misc.py:141-167 for an allocation >= 1: every entry is rounded"""
    idx = np.argsort(sol, kind="stable")
    idx = np.array([i for i in idx if sol[i] > 1.0e-8], dtype=np.int64)
    lb, ub = np.floor(sol).astype(int)[idx], np.ceil(sol).astype(int)[idx]
    order = np.argsort(lb, kind="stable")[::-1]
    return lb[order], ub[order], idx[order]


def mfmc_round_from_combo(sol, combo):
    """the integer point of combination `combo` of misc.py:390-393 (bit j: upper bound of the j-th bound entry)"""
    lb, ub, idx = mfmc_integer_bounds(sol)
    val = np.round(sol).astype(int)
    bits = (int(combo) >> np.arange(len(idx))) & 1
    val[idx] = np.where(bits == 1, ub, lb)
    return val


def _mfmc_sorted(sigmas, rhos, costs):
    idx = mfmc_order(rhos)
    s, w = sigmas[idx], costs[idx]
    rho = np.concatenate([rhos[idx], [0]])
    cost_ratio = w[:-1] / w[1:]
    with np.errstate(divide="ignore", invalid="ignore"):
        rho_ratio = (rho[:-2]**2 - rho[1:-1]**2) / (rho[1:-1]**2 - rho[2:]**2)
    feasible = bool(np.all(cost_ratio > rho_ratio))
    alphas = rho[1:-1] * s[0] / s[1:]
    return idx, s, rho, w, alphas, feasible


def _mfmc_variance(s, rho, alphas):
    def variance(m):
        with np.errstate(divide="ignore", invalid="ignore"):
            return s[0]**2 / m[0] + sum((1 / m[:-1] - 1 / m[1:]) * (alphas**2 * s[1:]**2 - 2 * alphas * rho[1:-1] * s[0] * s[1:]))
    return variance


def mfmc_allocation(sigmas, rhos, costs, budget=None, eps=None):
    """misc.py:90-107: (feasible, models in |rho| order, continuous allocation >= 1 in that order, variance callable, alphas)"""
    if budget is None and eps is None:
        raise ValueError("Need to specify either budget or RMSE tolerance")
    elif budget is not None and eps is not None:
        eps = None
    idx, s, rho, w, alphas, feasible = _mfmc_sorted(sigmas, rhos, costs)
    if not feasible:
        return False, idx, None, None, alphas
    r = np.sqrt(w[0] / w * (rho[:-1]**2 - rho[1:]**2) / (1 - rho[1]**2))
    if budget is not None: m1 = budget / (w @ r)
    else:                  m1 = eps**-2 * (w @ r) * (s[0]**2 / w[0]) * (1 - rho[1]**2)
    m = np.maximum(np.concatenate([[m1], m1 * r[1:]]), 1)
    return True, idx, m, _mfmc_variance(s, rho, alphas), alphas


def mfmc_low_budget_integer_solution(rhos, costs, budget):
    """misc.py:416-449 (Gruber et al. 2022, low-budget MFMC sample sizes)"""
    if rhos.shape[0] == 1:
        return np.array([np.floor(budget / costs[0])]).astype(np.int64)
    rho = np.concatenate([rhos, [0]])
    denom = rho[0] ** 2 - rho[1] ** 2
    r = np.sqrt(costs[0] / costs * (rho[:-1] ** 2 - rho[1:] ** 2) / denom)
    m1 = budget / (costs @ r)
    m = np.concatenate([[m1], m1 * r[1:]])
    if m[0] >= 1:
        return np.floor(m).astype(np.int64)
    m[0] = 1
    m[1:] = mfmc_low_budget_integer_solution(rhos=rhos[1:], costs=costs[1:], budget=budget - costs[0])
    return m.astype(np.int64)


def _best_closest_integer_solution(sol, obj, constr):
    """misc.py:384-413 with every candidate evaluated (argmin: the first minimum in combination order)"""
    lb, ub, idx = mfmc_integer_bounds(sol)
    LL = len(idx)
    if LL > 24:
        raise ValueError('Too many dimensions to brute-force it')
    fvals = np.full(2**LL, np.inf)
    for c in range(2**LL):
        val = mfmc_round_from_combo(sol, c)
        if constr(val): fvals[c] = obj(val)
    c = int(np.argmin(fvals))
    return mfmc_round_from_combo(sol, c), fvals[c]


def attempt_mfmc_setup(sigmas, rhos, costs, budget=None, eps=None, continuous_relaxation=False, small_budget=False):
    """misc.py:78-130: (feasible, {"samples", "error", "total_cost", "alphas", "variance"}), samples in |rho| order.
    small_budget: the low-budget scheme is applied in |rho| order (the reference passes the unsorted arrays; the two agree
    when model order follows |rho|)"""
    if budget is not None and eps is not None:
        eps = None
    sigmas, rhos, costs = (np.asarray(a, dtype=np.float64) for a in (sigmas, rhos, costs))
    if not all(np.isfinite(sigmas)): return False, None
    feasible, idx, m, variance, alphas = mfmc_allocation(sigmas, rhos, costs, budget=budget, eps=eps)
    if not feasible: return False, None
    w = costs[idx]
    if budget is not None:
        constraint = lambda m: m @ w <= budget and m[0] >= 1 and all(m[:-1] <= m[1:])
        obj = variance
    else:
        constraint = lambda m: variance(m) <= eps**2 and m[0] >= 1 and all(m[:-1] <= m[1:])
        obj = lambda m: m @ w
    if not continuous_relaxation:
        if small_budget and budget is not None:
            m = mfmc_low_budget_integer_solution(rhos[idx], w, budget)
        else:
            m, fval = _best_closest_integer_solution(m, obj, constraint)
            if np.isinf(fval): return False, None
    return True, {"samples": m, "error": np.sqrt(variance(m)), "total_cost": m @ w, "alphas": alphas, "variance": variance}


def compute_mfmc_data(sigmas, rhos, costs, samples):
    """misc.py:48-76: the MFMC estimator of given samples (listed in the models' order; returned in |rho| order)"""
    sigmas, rhos, costs = (np.asarray(a, dtype=np.float64) for a in (sigmas, rhos, costs))
    if not all(np.isfinite(sigmas)): return False, None
    idx, s, rho, w, alphas, feasible = _mfmc_sorted(sigmas, rhos, costs)
    if not feasible: return False, None
    m = np.array(samples)[idx]
    variance = _mfmc_variance(s, rho, alphas)(m)
    return True, {"samples": m, "error": np.sqrt(variance), "total_cost": m @ w, "alphas": alphas, "variance": variance}


# ---- MLMC (bluest/misc.py:15-46; bluest/blue_models.py:689-704): numpy mirrors for ONE model group ---------------------
# O(L) each (the brute-force rounding O(2^L)); the search over groups is bluest_mlmc_search (csrc/mlmc.hip).

def mlmc_levels(C, dV, w, group):
    """blue_models.py:689-704: (v, c), the level variances and level costs of `group` (model 0 first, by decreasing cost).
    Level i couples group[i] with group[i+1]; dV[min, max] replaces its variance where finite; the last level is the last
    model alone"""
    group = [int(g) for g in group]
    subC = np.asarray(C, dtype=np.float64)[np.ix_(group, group)]
    subw = np.asarray(w, dtype=np.float64)[group].copy()
    if len(group) > 1:
        v, corrs = np.diag(subC).copy(), np.diag(subC, 1)
        v[:-1] += v[1:] - 2 * corrs
        for i in range(len(group) - 1):
            check = dV[min(group[i], group[i + 1]), max(group[i], group[i + 1])]
            if np.isfinite(check):
                v[i] = check
        subw[:-1] += subw[1:]
    else:
        v = subC[0].copy()
    return v, subw


def mlmc_allocation(v, w, budget=None, eps=None):
    """misc.py:23-29: (continuous allocation >= 1, variance callable)"""
    with np.errstate(divide="ignore", invalid="ignore"):
        q = sum(np.sqrt(v * w))
        mu = budget / q if budget is not None else q / eps**2
        m = np.maximum(mu * np.sqrt(v / w), 1)
    return m, lambda m: sum(v[m > 0] / m[m > 0])


def attempt_mlmc_setup(v, w, budget=None, eps=None, continuous_relaxation=False):
    """misc.py:15-46: (feasible, {"samples", "error", "total_cost", "variance"}) for level variances v and level costs w"""
    if budget is None and eps is None:
        raise ValueError("Need to specify either budget or RMSE tolerance")
    elif budget is not None and eps is not None:
        eps = None
    v, w = np.asarray(v, dtype=np.float64), np.asarray(w, dtype=np.float64)
    if not all(np.isfinite(v)): return False, None
    m, variance = mlmc_allocation(v, w, budget=budget, eps=eps)
    if budget is not None:
        constraint = lambda m: m @ w <= budget and all(m >= 1)
        obj = variance
    else:
        constraint = lambda m: variance(m) <= eps**2 and all(m >= 1)
        obj = lambda m: m @ w
    if not continuous_relaxation:
        m, fval = _best_closest_integer_solution(m, obj, constraint)
        if np.isinf(fval): return False, None
    return True, {"samples": m, "error": np.sqrt(variance(m)), "total_cost": m @ w, "variance": variance}

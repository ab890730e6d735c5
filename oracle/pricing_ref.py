"""
The three small kernels around the Newton master of the second-order finish (csrc/newton.hip: k_price, k_support_point,
k_ma_update) restated in plain Python at the kernels' own arguments.  Nothing of bluest_amd is imported.

`price`, `support_point` and `ma_update` take what the kernels take (the plan's part of it -- L, n_out, goff, invmap, the v
workspace, N -- spelled out) and return what they must write.  Arithmetic: float64, the kernels' expressions operation by
operation.  +, *, / of Python floats are correctly rounded as on the device; a fused multiply-add is `fma`, evaluated exactly
in rationals and rounded once.  What is decided besides is discrete (guards, the first strict maximum of a thread's scan, the
tie rule of the workgroup's top 16), so the agreement expected of bluest_price* is exact: every reported value and index.

The reporting scheme of k_price: 64 workgroups of 256 threads; thread t of workgroup b scans i = b*256 + t, + 64*256, ...
ascending and keeps its first strict maximum; the workgroup reports the 16 largest of its 256 per-thread maxima, equal values
by ascending index, empty slots (-inf, -1) last.  Two of a workgroup's true top 16 on one thread's stride yield one candidate.
"""
import math
from fractions import Fraction

import numpy as np

PRICE_TOP, PRICE_BLOCKS, PRICE_THREADS = 16, 64, 256
PRICE_STRIDE = PRICE_BLOCKS * PRICE_THREADS
PRICE_CANDIDATES = PRICE_TOP * PRICE_BLOCKS
MAX_OUTPUTS = 64
EVAL_OK = 0
RC_OK, ERR_ARG, ERR_STATE = 0, 1, 4
DBL_EPS = 2.0 ** -52
# ulp bound of the device pow(): the ROCm device library implements the OpenCL full profile, which allows pow 16 ulp
POW_ULPS = 16.0
NEG_INF = float("-inf")


def fma(a, b, c):
    """a * b + c rounded once (Python converts a Fraction to the nearest float); IEEE special values as the hardware has them"""
    a, b, c = float(a), float(b), float(c)
    if not (math.isfinite(a) and math.isfinite(b) and math.isfinite(c)):
        return a * b + c                       # nan / inf: nothing to round (inf * 0 and inf - inf are nan either way)
    r = float(Fraction(a) * Fraction(b) + Fraction(c))
    if r == 0.0:                               # the sign of an exact zero: that of the float expression
        return a * b + c
    return r


def _local(invmap, o, i):
    return i if invmap is None else int(invmap[o][i])


def reduced_cost(i, n_out, grad, goff, invmap, mu, s, cc, capmask=None, nu=None, F2=0.0, terms=None):
    """c_i as k_price writes it: the fma chain over the outputs in output order (li < 0 and mu_o <= 0 skipped), one product
    with cc_i, with caps the correction summed over the set bits in ascending order and one fma.  `terms` (a list) receives the
    absolute values of the chain's products, for error bounds"""
    c = 0.0
    for o in range(n_out):
        li = _local(invmap, o, i)
        if li >= 0 and mu[o] > 0.0:
            a, g = mu[o] / s[o], -float(grad[int(goff[o]) + li])
            c = fma(a, g, c)
            if terms is not None:
                terms.append(abs(a * g))
    c = c * cc[i]
    if capmask is not None:
        mk, corr, b = int(capmask[i]), 0.0, 0
        while mk:
            if mk & 1:
                corr = corr + nu[b]
            mk >>= 1
            b += 1
        c = fma(-cc[i] * F2, corr, c)
    return c


def report(c):
    """(top_val, top_idx) of the 64 workgroups, PRICE_TOP entries each, from the reduced costs of all L groups"""
    L = len(c)
    top_val = np.full(PRICE_CANDIDATES, NEG_INF)
    top_idx = np.full(PRICE_CANDIDATES, -1, dtype=np.int64)
    for b in range(PRICE_BLOCKS):
        mine = []
        for t in range(PRICE_THREADS):
            best, besti = NEG_INF, -1
            for i in range(b * PRICE_THREADS + t, L, PRICE_STRIDE):
                if c[i] > best:
                    best, besti = c[i], i
            if besti >= 0:
                mine.append((-best, besti))
        mine.sort()                                                 # value descending, then index ascending
        for r, (nv, ix) in enumerate(mine[:PRICE_TOP]):
            top_val[b * PRICE_TOP + r], top_idx[b * PRICE_TOP + r] = -nv, ix
    return top_val, top_idx


def price(L, n_out, grad, goff, invmap, mu, s, cc, S, sup, v_ws, N, capmask=None, nu=None, master_out=None):
    """dict c (all L reduced costs), c_sup (S), top_val / top_idx (1024), y0 (n_out) -- the last four are the kernel's outputs"""
    F2 = float(master_out[0]) * float(master_out[0]) if capmask is not None else 0.0
    mu, s, cc = [float(x) for x in mu], [float(x) for x in s], [float(x) for x in cc]
    nu = None if nu is None else [float(x) for x in nu]
    c = np.array([reduced_cost(i, n_out, grad, goff, invmap, mu, s, cc, capmask, nu, F2) for i in range(L)])
    top_val, top_idx = report(c)
    return {"c": c, "c_sup": np.array([c[int(i)] for i in sup[:S]]), "top_val": top_val, "top_idx": top_idx,
            "y0": np.array([float(v_ws[o * N]) for o in range(n_out)])}


def bound(res, mu, s, S):
    """(cmax, A, lb) as the column generation reduces one pricing round (uncapped): cmax over the reported candidates and the
    support's own reduced costs, A = 2 sum_o (mu_o/s_o) y0_o, lb = A^2 / (4 cmax)"""
    a = np.asarray(mu, dtype=np.float64) / np.asarray(s, dtype=np.float64)
    A = 2.0 * float(a @ res["y0"])
    cmax = max(float(res["top_val"].max()), float(res["c_sup"][:S].max()))
    return cmax, A, (A * A / (4.0 * cmax) if cmax > 0.0 else 0.0)


def support_point(L, S, sup, xs, cc, eps):
    """m_i = cc_i ((1 - eps) x_S[i in S] + eps / L) in both roundings the compiler's default contraction allows for the inner
    expression: (separate multiply and add, one fma)"""
    pos = {int(g): j for j, g in enumerate(sup[:S])}
    one, bg = 1.0 - eps, eps / float(L)
    sep, fused = np.empty(L), np.empty(L)
    for i in range(L):
        xi = float(xs[pos[i]]) if i in pos else 0.0
        sep[i] = float(cc[i]) * (one * xi + bg)
        fused[i] = float(cc[i]) * fma(one, xi, bg)
    return sep, fused


def _pow(x, y):
    """x ** y correctly rounded when y is a small non-negative integer (p = 32 ships: y = 31), the host's pow otherwise"""
    if y == int(y) and 0 <= y <= 64 and math.isfinite(x):
        return float(Fraction(x) ** int(y))
    return math.pow(x, y)


def ma_update(L, n_out, var, status, grad, goff, invmap, s, cc, p, x, m):
    """(x, m) after one multiplicative step, and facts: evaluable, the weights, den.  Not evaluable (a status not OK, r_max not
    positive and finite): both come back as they were"""
    r = [float(var[o]) / float(s[o]) for o in range(n_out)]
    rmax, ok = 0.0, True
    for o in range(n_out):
        ok = ok and int(status[o]) == EVAL_OK
        if r[o] > rmax:                                             # fmax: a NaN never replaces the maximum
            rmax = r[o]
    ok = ok and rmax > 0.0 and math.isfinite(rmax)
    w = [1.0 if (n_out == 1 or not ok) else _pow(r[o] / rmax, p - 1.0) for o in range(n_out)]
    facts = {"ok": ok, "w": w, "r": r}
    x, m = np.array(x, dtype=np.float64), np.array(m, dtype=np.float64)
    if not ok:
        return x, m, facts
    den = 0.0
    for o in range(n_out):
        den = fma(w[o], r[o], den)
    wgt = [w[o] / float(s[o]) for o in range(n_out)]
    facts["den"] = den
    for i in range(L):
        num = 0.0
        for o in range(n_out):
            li = _local(invmap, o, i)
            if li >= 0:
                num = fma(wgt[o], -float(grad[int(goff[o]) + li]), num)
        xn = float(x[i]) * float(cc[i]) * num / den
        x[i] = xn
        m[i] = float(cc[i]) * xn
    return x, m, facts

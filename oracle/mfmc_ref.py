"""
The MFMC model-subset search (csrc/mfmc.hip: bluest_mfmc_search) restated in numpy at the kernel's own interface.

`search` takes the arguments of the C entry point and returns what it must write, plus a `facts` record that says which paths
of the kernel the input drives and how far every discrete decision on the way is from flipping.  It restates
bluest/misc.py:78-175, 384-449 and bluest/blue_models.py:797-865 on its own: nothing of bluest_amd is imported.

Cliques through model 0 are enumerated from `adj` by extension (size first, then lexicographic: the order of
networkx.enumerate_all_cliques), never by scanning the 2^nb masks, so a sparse graph costs what its cliques cost.

Arithmetic: float64, the kernel's expressions operation by operation, every dot product summed sequentially from i = 0
(no `@`, no BLAS).  The cliques of one size are evaluated together, one numpy operation per kernel operation; each of those
(+, -, *, /, sqrt, floor, ceil) is correctly rounded here as on the device, the kernel is compiled without contraction, and
all that is decided is discrete (feasibility, monotone order, floor/ceil, argmin).  So the agreement expected is exact,
best_obj included.

Rounding: the kernel tries all 2^L floor/ceil combinations of a clique.  Positions whose floor equals their ceil give the
same point for either bit, and the first minimum in increasing combination index has those bits clear; so only positions with
floor != ceil are enumerated (`full=True` enumerates all 2^L; the CPU tests compare the two).
"""
import math
from itertools import combinations

import numpy as np

MAX_NEIGHBOURS, MAX_ROUND, MAX_OUTPUTS = 30, 24, 64
BUDGET, CONTINUOUS, SMALL_BUDGET = 1, 2, 4
OK, NONE, TOO_BIG = 0, 1, 2
RC_OK, ERR_ARG, ERR_STATE = 0, 1, 4
CAND_CAP = 1 << 16
LB_MARGIN_MIN, LB_MARGIN_ULPS = 1e-9, 16.0
DBL_EPS = 2.0 ** -52
# the host window loop (mfmc.hip): halvings per window, counting scans between two windows that round something
MAX_HALVINGS, MAX_IDLE_SCANS = 200, 4096
INF = float("inf")


class Result(object):
    """rc: return code; status, best_mask, best_combo[n_out], best_obj: the outputs (None when rc != 0: nothing is written)"""

    def __init__(self, rc, status=None, best_mask=None, best_combo=None, best_obj=None, facts=None):
        self.rc, self.status, self.best_mask, self.best_combo, self.best_obj = rc, status, best_mask, best_combo, best_obj
        self.facts = facts if facts is not None else {}


class _Prob(object):
    pass


def _margin(F, name, values):
    """record the smallest of `values` (relative distances of a decision from flipping); NaN and inf are decisions that no
    rounding can flip (a comparison with an exact 0/0 or x/0)"""
    v = np.asarray(values, dtype=np.float64).ravel()
    v = v[np.isfinite(v)]
    if v.size:
        F["margins"][name] = min(F["margins"].get(name, INF), float(v.min()))


def _rel_gap(a, b):
    with np.errstate(divide="ignore", invalid="ignore"):
        return np.abs(a - b) / np.maximum(np.abs(a), np.abs(b))


def enumerate_cliques(nb, adj):
    """cliques through model 0 as neighbour bitmasks, one uint32 array per size (index = number of neighbours), each in
    lexicographic order: a clique extends by every neighbour above its last one that is adjacent to all of it"""
    adj = [int(a) for a in (adj if adj is not None else [])]
    levels = [np.zeros(1, dtype=np.uint32)]
    cur = [(0, (1 << nb) - 1)]                                  # (mask, neighbours that may still extend it)
    while True:
        nxt = []
        for mask, ext in cur:
            e = ext
            while e:
                b = (e & -e).bit_length() - 1
                e &= e - 1
                nxt.append((mask | (1 << b), ext & adj[b] & ~((2 << b) - 1)))
        if not nxt:
            return levels
        levels.append(np.array([m for m, _ in nxt], dtype=np.uint32))
        cur = nxt


def _has_big_clique(P):
    """does a clique with more than MAX_ROUND models pass output 0's ordering test?  (The kernel meets it in its scan; here
    such cliques are looked for directly, in the core of neighbours with at least MAX_ROUND - 1 neighbours of their own, so
    that the 2^24 cliques below them need not be enumerated.  The subsets of that core are tried one by one: cheap when the
    core is barely larger than MAX_ROUND or its first large subset is feasible, exponential for a dense graph of 30
    neighbours whose large cliques all fail the ordering test -- keep such inputs out of the case table.)"""
    need = MAX_ROUND                                            # neighbours in the clique
    if P.nb < need: return False
    alive = (1 << P.nb) - 1
    while True:
        drop = 0
        for b in range(P.nb):
            if (alive >> b) & 1 and bin(P.adj[b] & alive).count("1") < need - 1: drop |= 1 << b
        if not drop: break
        alive &= ~drop
    core = [b for b in range(P.nb) if (alive >> b) & 1]
    for size in range(need, len(core) + 1):
        for sub in combinations(core, size):
            mask = sum(1 << b for b in sub)
            if all((mask & ~(P.adj[b] | (1 << b))) == 0 for b in sub):
                if _Views(P, np.array([mask], dtype=np.uint32), size + 1, 0).feasible(None)[0]: return True
    return False


class _Views(object):
    """output n of the cliques `masks` (all of L models): models in |rho| order, one row per clique (the kernel's View)"""

    def __init__(self, P, masks, L, n):
        self.P, self.L, self.n, nc = P, L, n, len(masks)
        members = np.zeros((nc, L), dtype=np.int64)
        if L > 1:
            bits = (masks[:, None] >> np.arange(P.nb, dtype=np.uint32)[None, :]) & 1
            members[:, 1:] = np.nonzero(bits)[1].reshape(nc, L - 1) + 1
        order = np.argsort(P.rank[n][members], axis=1, kind="stable")
        self.q = np.take_along_axis(members, order, axis=1)
        self.rho = np.zeros((nc, L + 2))
        self.rho[:, :L] = P.rho[n][self.q]
        self.sig, self.w = P.s[n][self.q], P.w[self.q]
        self.s0, self.r1 = self.sig[:, 0], self.rho[:, 1]

    def feasible(self, F):
        ok = np.ones(len(self.q), dtype=bool)
        for i in range(self.L - 1):
            a, b, c = self.rho[:, i], self.rho[:, i + 1], self.rho[:, i + 2]
            cr = self.w[:, i] / self.w[:, i + 1]
            rr = (a * a - b * b) / (b * b - c * c)
            if F is not None: _margin(F, "cost_ratio_vs_rho_ratio", _rel_gap(cr, rr)[ok])
            ok &= cr > rr
        return ok

    def r(self, i):
        a, b = self.rho[:, i], self.rho[:, i + 1]
        return np.sqrt(((self.w[:, 0] / self.w[:, i]) * (a * a - b * b)) / (1.0 - self.r1 * self.r1))

    def m1(self):
        dot = np.zeros(len(self.q))
        for i in range(self.L): dot = dot + self.w[:, i] * self.r(i)
        if self.P.budget_mode: return self.P.budget / dot
        return ((self.P.epsm2[self.n] * dot) * ((self.s0 * self.s0) / self.w[:, 0])) * (1.0 - self.r1 * self.r1)

    def m_raw(self, m1):
        return np.stack([m1 if i == 0 else m1 * self.r(i) for i in range(self.L)], axis=1)

    def coef(self, i):
        si, ri = self.sig[:, i], self.rho[:, i]
        al = (ri * self.s0) / si
        return (al * al) * (si * si) - (((2.0 * al) * ri) * self.s0) * si

    def variance(self, m):
        """m: (rows, L), rows aligned with the cliques"""
        total = np.zeros(m.shape[0])
        for i in range(1, self.L):
            total = total + (1.0 / m[:, i - 1] - 1.0 / m[:, i]) * self.coef(i)
        return (self.s0 * self.s0) / m[:, 0] + total

    def cost(self, m):
        c = np.zeros(m.shape[0])
        for i in range(self.L): c = c + m[:, i] * self.w[:, i]
        return c

    def lower_bound(self):
        Q = np.zeros(len(self.q))
        for i in range(self.L):
            a = 1.0 - self.r1 * self.r1 if i == 0 else self.rho[:, i] * self.rho[:, i] - self.rho[:, i + 1] * self.rho[:, i + 1]
            Q = Q + np.sqrt(np.fmax(a, 0.0) * self.w[:, i])
        s0 = self.s0
        v = np.sqrt((s0 * s0) * (Q * Q) / self.P.budget) if self.P.budget_mode else (Q * Q) * (s0 * s0) / self.P.eps2[self.n]
        margin = np.fmax(LB_MARGIN_MIN, LB_MARGIN_ULPS * self.L * DBL_EPS / (1.0 - self.r1 * self.r1))
        return np.where(margin < 1.0, v * (1.0 - margin), 0.0)

    def take(self, rows):
        V = object.__new__(_Views)
        V.P, V.L, V.n = self.P, self.L, self.n
        for k in ("q", "rho", "sig", "w", "s0", "r1"): setattr(V, k, getattr(self, k)[rows])
        return V


def _monotone(m):
    ok = m[:, 0] >= 1.0
    for i in range(1, m.shape[1]): ok &= m[:, i - 1] <= m[:, i]
    return ok


def _low_budget(rho, w, L, budget, F):
    """misc.py:416-449 for one clique in |rho| order (rho padded with zeros): (m, number of leading models pinned to 1)"""
    m, start = np.zeros(L), 0
    while True:
        if L - start == 1:
            x = budget / w[start]
            _margin(F, "m_to_integer", [abs(x - round(x)) / abs(x)] if math.isfinite(x) and x != 0 else [])
            m[start] = math.floor(x) if math.isfinite(x) else x
            return m, start
        denom = rho[start] * rho[start] - rho[start + 1] * rho[start + 1]
        with np.errstate(divide="ignore", invalid="ignore"):
            r = [np.sqrt(((w[start] / w[i]) * (rho[i] * rho[i] - rho[i + 1] * rho[i + 1])) / denom) for i in range(start, L)]
            dot = 0.0
            for i in range(start, L): dot = dot + w[i] * r[i - start]
            m1 = budget / dot
        _margin(F, "m_to_integer", [abs(m1 - 1.0)])
        if m1 >= 1.0:
            for i in range(start, L):
                x = m1 if i == start else m1 * r[i - start]
                _margin(F, "m_to_integer", [abs(x - round(x)) / abs(x)] if math.isfinite(x) else [])
                m[i] = np.floor(x)
            return m, start
        m[start] = 1.0
        budget = budget - w[start]
        start += 1


def _nan_max(worst, err):
    return np.where((err > worst) | (err != err), err, worst)


def _scan_level(P, masks, L, F):
    """eval_clique for the cliques of one size: dict of arrays over `masks`"""
    nc = len(masks)
    out = {"ok": np.ones(nc, dtype=bool), "obj": np.full(nc, INF), "lb": np.full(nc, INF), "ub": np.full(nc, INF)}
    eps_mode = not P.budget_mode
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        views = [_Views(P, masks, L, n) for n in range(P.n_out)]
        for V in views: out["ok"] &= V.feasible(F)
        keep = np.flatnonzero(out["ok"])
        if keep.size == 0: return out
        views = [V.take(keep) for V in views]
        k = keep.size
        mx = np.zeros((k, P.nb + 1))
        rows = np.arange(k)
        worst, lbmax, ub_ok = np.zeros(k), np.zeros(k), np.ones(k, dtype=bool)
        for V in views:
            m1 = V.m1()
            if P.integer_round:
                lbmax = np.fmax(lbmax, V.lower_bound())
                raw = V.m_raw(m1)
                m = np.fmax(raw, 1.0)
                # floor/ceil and the clamp at 1 are decisions: distance of the unclamped m to the nearest integer (to 1 below 1)
                d = np.where(raw < 1.0, 1.0 - raw, np.abs(m - np.round(m)) / m)
                _margin(F, "m_to_integer", d[np.isfinite(raw) & (d > 0.0)])
                F["m_exact_integers"] += int(np.count_nonzero((d == 0.0) & np.isfinite(raw) & (m != 1.0)))
                mr = np.floor(m) if P.budget_mode else np.ceil(m)
                ok = _monotone(mr)
                cost, var = V.cost(mr), V.variance(mr)
                if P.budget_mode:
                    _margin(F, "cost_vs_budget", _rel_gap(cost, P.budget)[ok])
                    ok &= cost <= P.budget
                else:
                    _margin(F, "var_vs_eps2", _rel_gap(var, P.eps2[V.n])[ok])
                    ok &= var <= P.eps2[V.n]
                ub_ok &= ok
                if eps_mode:
                    for i in range(L): mx[rows, V.q[:, i]] = np.fmax(mx[rows, V.q[:, i]], mr[:, i])
                else:
                    worst = np.fmax(worst, np.sqrt(var))
            elif P.budget_mode and P.small_budget:
                err = np.empty(k)
                for j in range(k):
                    mj, pins = _low_budget(V.rho[j], V.w[j], L, P.budget, F)
                    F["pins"].add((L, pins))
                    err[j] = np.sqrt(V.take([j]).variance(mj[None, :]))[0]
                worst = _nan_max(worst, err)
            else:
                mc = np.fmax(V.m_raw(m1), 1.0)
                if eps_mode:
                    for i in range(L): mx[rows, V.q[:, i]] = np.fmax(mx[rows, V.q[:, i]], mc[:, i])
                else:
                    worst = _nan_max(worst, np.sqrt(V.variance(mc)))
        obj = worst
        if eps_mode:
            V = views[0]
            obj = np.zeros(k)
            for i in range(L): obj = obj + mx[rows, V.q[:, i]] * V.w[:, i]
        obj = np.where(obj != obj, INF, obj)
        if P.integer_round:
            out["lb"][keep] = lbmax
            out["ub"][keep] = np.where(ub_ok, obj, INF)
        else:
            out["obj"][keep] = obj
    return out


def _bounds(V, m):
    """lb, ub and the position of each bound entry (get_feasible_integer_bounds, misc.py:141-167): entry j of the 2^L
    combinations rounds position pos[:, j]"""
    lb, ub = np.floor(m), np.ceil(m)
    idx = np.argsort(m, axis=1, kind="stable")
    ord2 = np.argsort(np.take_along_axis(lb, idx, axis=1), axis=1, kind="stable")
    pos = np.take_along_axis(idx, ord2[:, ::-1], axis=1)
    return lb, ub, pos


def _round_output(P, V, F, full):
    """k_mfmc_round for output V.n of the cliques of V: (fval, combo, the chosen point per position)"""
    k, L = len(V.q), V.L
    m = np.fmax(V.m_raw(V.m1()), 1.0)
    lb, ub, pos = _bounds(V, m)
    fval, combo, point = np.full(k, INF), np.zeros(k, dtype=np.uint32), lb.copy()
    rows_all = np.arange(k)
    frac = np.take_along_axis(lb != ub, pos, axis=1)                    # per bound entry j
    nfrac = np.full(k, L) if full else frac.sum(axis=1)
    for nf in np.unique(nfrac):
        sel = rows_all[nfrac == nf]
        Vs, g = V.take(sel), len(sel)
        # the entries to enumerate, in increasing j: sub-combination t maps to increasing c
        js = np.tile(np.arange(L), (g, 1)) if full else np.nonzero(frac[sel])[1].reshape(g, nf)
        ps = np.take_along_axis(pos[sel], js, axis=1)
        bf, bc, bp = np.full(g, INF), np.zeros(g, dtype=np.uint32), lb[sel].copy()
        rg = np.arange(g)
        for t in range(1 << int(nf)):
            pt = lb[sel].copy()
            c = np.zeros(g, dtype=np.uint32)
            for b in range(int(nf)):
                if (t >> b) & 1:
                    pt[rg, ps[:, b]] = ub[sel][rg, ps[:, b]]
                    c |= (np.uint32(1) << js[:, b].astype(np.uint32))
            ok = _monotone(pt)
            cost, var = Vs.cost(pt), Vs.variance(pt)
            if P.budget_mode:
                _margin(F, "cost_vs_budget", _rel_gap(cost, P.budget)[ok])
                f = np.where(ok & (cost <= P.budget), var, INF)
            else:
                _margin(F, "var_vs_eps2", _rel_gap(var, P.eps2[V.n])[ok])
                f = np.where(ok & (var <= P.eps2[V.n]), cost, INF)
            win = f < bf
            bf, bc = np.where(win, f, bf), np.where(win, c, bc)
            bp[win] = pt[win]
        fval[sel], combo[sel], point[sel] = bf, np.where(bf < INF, bc, 0).astype(np.uint32), bp
    return fval, combo, point


def combination_values(P, mask, L, n):
    """every one of the 2^L combinations of one clique and one output, as k_mfmc_round's lanes see them: (f[2^L], the bound
    entries j whose floor equals their ceil)"""
    V1 = _Views(P, np.array([mask], dtype=np.uint32), L, n)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        lb, ub, pos = _bounds(V1, np.fmax(V1.m_raw(V1.m1()), 1.0))
        c = np.arange(1 << L)
        V = V1.take(np.zeros(1 << L, dtype=np.int64))
        pt = np.tile(lb, (1 << L, 1))
        for j in range(L):
            up = ((c >> j) & 1) == 1
            pt[up, pos[0, j]] = ub[0, pos[0, j]]
        ok, cost, var = _monotone(pt), V.cost(pt), V.variance(pt)
        f = np.where(ok & (cost <= P.budget), var, INF) if P.budget_mode else np.where(ok & (var <= P.eps2[n]), cost, INF)
    return f, [j for j in range(L) if lb[0, pos[0, j]] == ub[0, pos[0, j]]]


def last_minimum_combo(f, lanes=256):
    """what k_mfmc_round would return if each lane kept the LAST of its equal minima (lane t sees c = t, t + 256, ...), the
    lanes still merged by (value, lowest index).  The kernel must keep the first; where the two differ a test can tell."""
    best = (INF, 0)
    for t in range(min(lanes, len(f))):
        own = f[t::lanes]
        k = len(own) - 1 - int(np.argmin(own[::-1]))
        best = min(best, (float(own[k]), t + lanes * k))
    return best[1]


def _round_level(P, masks, L, F, full):
    """k_mfmc_round for candidate cliques of one size: (obj, combo[k, n_out])"""
    k = len(masks)
    combos = np.zeros((k, P.n_out), dtype=np.uint32)
    with np.errstate(divide="ignore", invalid="ignore", over="ignore"):
        views = [_Views(P, masks, L, n) for n in range(P.n_out)]
        mx, rows = np.zeros((k, P.nb + 1)), np.arange(k)
        ok, worst = np.ones(k, dtype=bool), np.zeros(k)
        for V in views:
            fval, combos[:, V.n], point = _round_output(P, V, F, full)
            ok &= fval < INF
            if P.budget_mode: worst = _nan_max(worst, np.sqrt(fval))
            else:
                for i in range(L): mx[rows, V.q[:, i]] = np.fmax(mx[rows, V.q[:, i]], point[:, i])
        obj = worst
        if not P.budget_mode:
            V, obj = views[0], np.zeros(k)
            for i in range(L): obj = obj + mx[rows, V.q[:, i]] * V.w[:, i]
        obj = np.where(ok & (obj == obj), obj, INF)
    return obj, combos


def _windows(lb, hi0, round_them, F):
    """the host window loop on the lower bounds of the scanned cliques: windows (lo, T] of at most CAND_CAP cliques, T halved
    until the count fits, `best` tightening the upper end.  `round_them(indices)` rounds the cliques of one window and
    returns their objectives.  Returns the return code; fills F["windows"] with (lo, T, cliques, halvings)."""
    order = np.argsort(lb, kind="stable")
    slb = lb[order]
    count = lambda a, b: int(np.searchsorted(slb, b, side="right") - np.searchsorted(slb, a, side="right"))
    lo, best, idle, wins = -1.0, INF, 0, []
    F["windows"], F["scans"] = wins, 0
    while True:
        hi = min(hi0, best)
        if not lo < hi: return RC_OK
        T, it = hi, 0
        c = count(lo, T); idle += 1; F["scans"] += 1
        while c > CAND_CAP:
            if it >= MAX_HALVINGS: return ERR_STATE
            T = lo + 0.5 * (T - lo)
            if not T > lo: break
            c = count(lo, T); idle += 1; F["scans"] += 1; it += 1
        if not T > lo or c > CAND_CAP or idle >= MAX_IDLE_SCANS: return ERR_STATE     # the cap: once per window
        if c > 0:
            a, b = np.searchsorted(slb, lo, side="right"), np.searchsorted(slb, T, side="right")
            best = min(best, float(round_them(order[a:b]).min()))
            idle = 0
        wins.append((lo, T, c, it))
        lo = T


def check_args(nb, n_out, flags, eps2, epsm2, w, s, rho, perm, adj, outputs_given=True):
    if nb < 0 or nb > MAX_NEIGHBOURS or n_out <= 0 or n_out > MAX_OUTPUTS: return ERR_ARG
    if w is None or s is None or rho is None or perm is None or (nb > 0 and adj is None) or not outputs_given: return ERR_ARG
    if not flags & BUDGET and (eps2 is None or epsm2 is None): return ERR_ARG
    pm = np.asarray(perm).reshape(n_out, nb + 1)
    if ((pm < 0) | (pm > nb)).any() or (pm[:, 0] != 0).any() or (pm[:, 1:] == 0).any(): return ERR_ARG
    return RC_OK


def search(nb, n_out, flags, budget, eps2, epsm2, w, s, rho, perm, adj, full=False, outputs_given=True):
    """bluest_mfmc_search: Result (rc, status, best_mask, best_combo, best_obj, facts)"""
    rc = check_args(nb, n_out, flags, eps2, epsm2, w, s, rho, perm, adj, outputs_given)
    if rc: return Result(rc)
    P = _Prob()
    P.nb, P.n_out, P.budget = nb, n_out, float(budget)
    P.budget_mode, P.continuous, P.small_budget = bool(flags & BUDGET), bool(flags & CONTINUOUS), bool(flags & SMALL_BUDGET)
    P.integer_round = not P.continuous and not (P.small_budget and P.budget_mode)
    P.w = np.asarray(w, dtype=np.float64).reshape(nb + 1)
    P.s, P.rho = (np.asarray(a, dtype=np.float64).reshape(n_out, nb + 1) for a in (s, rho))
    P.eps2, P.epsm2 = (None if a is None else np.asarray(a, dtype=np.float64) for a in (eps2, epsm2))
    P.perm = np.asarray(perm, dtype=np.int64).reshape(n_out, nb + 1)
    P.rank = np.empty_like(P.perm)
    for n in range(n_out): P.rank[n][P.perm[n]] = np.arange(nb + 1)
    P.adj = [int(a) for a in adj] if nb > 0 else []
    F = {"margins": {}, "pins": set(), "m_exact_integers": 0}
    if P.integer_round and _has_big_clique(P):
        F["too_big"] = True
        return Result(RC_OK, TOO_BIG, 0xffffffff, np.zeros(n_out, dtype=np.uint32), INF, F)

    levels = enumerate_cliques(nb, P.adj)
    masks = np.concatenate(levels)
    sizes = np.concatenate([np.full(len(lv), L + 1) for L, lv in enumerate(levels)])
    F["cliques"] = int(len(masks))
    ev = [_scan_level(P, lv, L + 1, F) for L, lv in enumerate(levels)]
    ok = np.concatenate([e["ok"] for e in ev])
    F["feasible"] = int(ok.sum())
    combos = np.zeros((len(masks), n_out), dtype=np.uint32)
    if not P.integer_round:
        obj = np.concatenate([e["obj"] for e in ev])
        lbs = obj
    else:
        lb, ub = np.concatenate([e["lb"] for e in ev]), np.concatenate([e["ub"] for e in ev])
        U = float(ub.min())
        LBmax = float(lb[np.isfinite(lb)].max()) if np.isfinite(lb).any() else 0.0
        hi0 = min(U, LBmax)
        cand = ok & (lb <= hi0)
        F["candidates"], F["min_ub"] = int(cand.sum()), U
        obj, rounded = np.full(len(masks), INF), np.zeros(len(masks), dtype=bool)

        def round_them(sel_all):
            for L in np.unique(sizes[sel_all]):
                sel = np.sort(sel_all[sizes[sel_all] == L])
                obj[sel], combos[sel] = _round_level(P, masks[sel], int(L), F, full)
            rounded[sel_all] = True
            return obj[sel_all]
        rc = _windows(np.where(ok, lb, INF), hi0, round_them, F)
        F["rounded"] = int(rounded.sum())
        if rc: return Result(rc, facts=F)
        lbs = np.where(rounded, obj, lb)                  # what each clique's objective is at least
    best = int(np.argmin(obj))                            # first minimum: ties go to the earlier clique
    if not obj[best] < INF:
        return Result(RC_OK, NONE, 0xffffffff, np.zeros(n_out, dtype=np.uint32), INF, F)
    F["winner_index"], F["winner_size"] = best, int(sizes[best])
    F["highest_bit"] = int(masks[best]).bit_length() - 1
    F["winner_combo"] = [int(c) for c in combos[best]]
    F["winner_all_ones"] = (1 << int(sizes[best])) - 1
    others = np.delete(lbs, best)
    F["runner_up_gap"] = float((others.min() - obj[best]) / obj[best]) if others.size and others.min() < INF else INF
    F["tied_masks"] = [int(m) for m in masks[obj == obj[best]] if int(m) != int(masks[best])]
    F["ties"] = len(F["tied_masks"])
    if P.integer_round:
        F["winner_is_min_ub"] = bool(ub[best] == U)
        F["winner_lb"] = float(lb[best])
        if sizes[best] <= 12:
            fs = [combination_values(P, int(masks[best]), int(sizes[best]), n) for n in range(n_out)]
            assert all(int(np.argmin(f)) == int(c) for (f, _), c in zip(fs, combos[best]))
            F["winner_clamped_entries"] = [cl for _, cl in fs]
            F["winner_last_minimum_combo"] = [last_minimum_combo(f) for f, _ in fs]
        F["winner_window"] = next((i for i, (a, b, _, _) in enumerate(F["windows"]) if a < lb[best] <= b), None)
    return Result(RC_OK, OK, int(masks[best]), combos[best].copy(), float(obj[best]), F)


# ------------------------------------------------------------------------------------------------------
# around the kernel: what BLUEProblem._mfmc_search does before and after it (blue_models.py:797-865)
# ------------------------------------------------------------------------------------------------------
def inputs_from_covariances(Cs, w, budget=None, eps=None, continuous_relaxation=False, small_budget=False):
    """the kernel's arguments for the covariances Cs (one per output; an infinite or zero entry: the pair is never coupled, the
    default of BLUEProblem) and costs w: dict of search()'s arguments, plus `local` (the model of each local index)"""
    Cs = [np.asarray(C, dtype=np.float64) for C in Cs]
    linked = np.ones(Cs[0].shape, dtype=bool)
    for C in Cs:
        coupled = ~np.isinf(C) & (C != 0.0)
        linked &= coupled & coupled.T
    np.fill_diagonal(linked, True)
    local = np.array([0] + [j for j in range(1, len(w)) if linked[0, j]])
    nb, n_out = len(local) - 1, len(Cs)
    s, rho = np.empty((n_out, nb + 1)), np.empty((n_out, nb + 1))
    for n, C in enumerate(Cs):
        sd = np.sqrt(np.diag(C))
        s[n], rho[n] = sd[local], (C[0] / (sd[0] * sd))[local]
    perm = np.array([np.argsort(np.abs(r), kind="stable")[::-1] for r in rho], dtype=np.int32)
    adj = np.array([sum(1 << (q - 1) for q in range(1, nb + 1) if q != p and linked[local[p], local[q]])
                    for p in range(1, nb + 1)], dtype=np.uint32)
    flags = (BUDGET if budget is not None else 0) | (CONTINUOUS if continuous_relaxation else 0) | (SMALL_BUDGET if small_budget else 0)
    if budget is None and np.isscalar(eps): eps = [eps] * n_out
    return dict(nb=nb, n_out=n_out, flags=flags, budget=float(budget or 0.0),
                eps2=None if budget is not None else np.array([e**2 for e in eps]),
                epsm2=None if budget is not None else np.array([e**-2 for e in eps]),
                w=np.asarray(w, dtype=np.float64)[local].copy(), s=s, rho=rho, perm=perm, adj=adj), local


def host_samples(args, local, mask, combo):
    """(models, samples) as setup_mfmc reports them for the kernel's answer: each output's allocation on the chosen clique
    (continuous, low-budget, or rounded by its combination), the per-model maximum, and the budget correction"""
    F = {"margins": {}, "pins": set(), "m_exact_integers": 0}
    P = _Prob()
    P.nb, P.n_out, P.budget = args["nb"], args["n_out"], args["budget"]
    P.budget_mode = bool(args["flags"] & BUDGET)
    P.w, P.s, P.rho, P.eps2, P.epsm2 = args["w"], args["s"], args["rho"], args["eps2"], args["epsm2"]
    P.rank = np.empty((P.n_out, P.nb + 1), dtype=np.int64)
    for n in range(P.n_out): P.rank[n][args["perm"][n]] = np.arange(P.nb + 1)
    L = bin(mask).count("1") + 1
    per_output = []
    with np.errstate(divide="ignore", invalid="ignore"):
        for n in range(P.n_out):
            V = _Views(P, np.array([mask], dtype=np.uint32), L, n)
            m = np.fmax(V.m_raw(V.m1()), 1.0)
            if not args["flags"] & CONTINUOUS:
                if args["flags"] & SMALL_BUDGET and P.budget_mode:
                    m = _low_budget(V.rho[0], V.w[0], L, P.budget, F)[0][None, :].astype(np.int64)
                else:
                    lb, ub, pos = _bounds(V, m)
                    m = lb.copy()
                    for j in range(L):
                        if (int(combo[n]) >> j) & 1: m[0, pos[0, j]] = ub[0, pos[0, j]]
                    m = m.astype(np.int64)
            per_output.append((V.q[0], m[0]))
    order = per_output[0][0]
    assert all(np.array_equal(q, order) for q, _ in per_output), "the outputs order the clique differently"
    samples = np.max(np.vstack([m for _, m in per_output]), axis=0)
    wm = P.w[order]
    if P.budget_mode:
        cost, ww = 0.0, 0.0
        for i in range(L): cost, ww = cost + samples[i] * wm[i], ww + wm[i] * wm[i]
        samples = np.floor(samples - (max(cost - P.budget, 0) / ww) * wm).astype(np.int64)
        samples[0] = max(samples[0], 1)
    return [int(local[q]) for q in order], samples

"""
The MLMC model-subset search (csrc/mlmc.hip: bluest_mlmc_search) restated in numpy at the kernel's own interface: exhaustive,
every admissible group rounded, no pruning.  Nothing of bluest_amd is imported.

`search` takes the arguments of the C entry point and returns what it must write, plus `facts` about the input (how many groups,
how many of them the kernel's bounds would keep, the winner's size, the ties).  It restates bluest/misc.py:15-46, 141-167,
384-413 and bluest/blue_models.py:662-723.

Admissible groups are enumerated from `adj` by depth-first search over paths from position 0, never by scanning the 2^nb masks,
and then ranked in the reference's order ([0], then by decreasing size, then the removed positions lexicographically).

Arithmetic: float64, the kernel's expressions operation by operation, every sum sequential from i = 0 (no `@`, no BLAS).  The
groups of one size are evaluated together, one numpy operation per kernel operation; each of those (+, *, /, sqrt, floor, ceil)
is correctly rounded here as on the device, the kernel is compiled without contraction, and all that is decided is discrete.
So the agreement expected is exact, best_obj included.

Rounding: the kernel tries all 2^L floor/ceil combinations of a group.  Positions whose floor equals their ceil give the same
point for either bit, and the first minimum in increasing combination index has those bits clear; so only positions with
floor != ceil are enumerated (`full=True` enumerates all 2^L; the CPU tests compare the two).
"""
import numpy as np

MAX_CANDIDATES, MAX_ROUND, MAX_OUTPUTS = 30, 24, 64
BUDGET, CONTINUOUS = 1, 2
OK, NONE, TOO_BIG = 0, 1, 2
RC_OK, ERR_ARG, ERR_STATE = 0, 1, 4
CAND_CAP = 1 << 16
INF = float("inf")


class Result(object):
    """rc: return code; status, best_mask, best_combo[n_out], best_obj: the outputs (None where nothing is written)"""

    def __init__(self, rc, status=None, best_mask=None, best_combo=None, best_obj=None, facts=None):
        self.rc, self.status, self.best_mask, self.best_combo, self.best_obj = rc, status, best_mask, best_combo, best_obj
        self.facts = facts if facts is not None else {}


def enumerate_groups(nb, adj):
    """admissible groups as bitmasks over positions 1..nb (bit p-1 = position p), by depth-first search over paths from 0"""
    adj = [int(a) for a in adj]
    out, stack = [0], [(0, 0)]                                  # (last position, mask)
    while stack:
        p, mask = stack.pop()
        ext = adj[p] >> (p + 1)
        q = p + 1
        while ext:
            if ext & 1:
                m = mask | (1 << (q - 1))
                out.append(m)
                stack.append((q, m))
            ext >>= 1
            q += 1
    return out


def order_key(mask, nb):
    """sort key of the reference's enumeration: [0] first, larger groups first, then the lowest differing position removed first"""
    rev = int(format(mask, "0%db" % max(nb, 1))[::-1], 2)
    return (mask != 0, -bin(mask).count("1"), rev)


def members_of(masks, L, nb):
    """(k, L) positions of the groups `masks`, all of L models"""
    masks = np.asarray(masks, dtype=np.uint32)
    members = np.zeros((len(masks), L), dtype=np.int64)
    if L > 1:
        bits = (masks[:, None] >> np.arange(nb, dtype=np.uint32)[None, :]) & 1
        members[:, 1:] = np.nonzero(bits)[1].reshape(len(masks), L - 1) + 1
    return members


class _Level(object):
    """output n of groups of L models: v, c (k, L) level variances and costs"""

    def __init__(self, P, members, n):
        L = members.shape[1]
        nxt = np.concatenate([members[:, 1:], members[:, -1:]], axis=1)
        self.v = P.lv[n][members, nxt]
        self.c = P.w[members] + np.where(np.arange(L)[None, :] < L - 1, P.w[nxt], 0.0)
        self.c[:, -1] = P.w[members[:, -1]]
        self.finite = np.isfinite(self.v).all(axis=1)
        q = np.zeros(len(members))
        for i in range(L): q = q + np.sqrt(self.v[:, i] * self.c[:, i])
        mu = P.budget / q if P.budget_mode else q / P.eps2[n]
        m = mu[:, None] * np.sqrt(self.v / self.c)
        self.m = np.where(m != m, m, np.fmax(m, 1.0))

    def variance(self, m):
        tot = np.zeros(m.shape[0])
        for i in range(m.shape[1]):
            tot = np.where(m[:, i] > 0.0, tot + self.v[:, i] / m[:, i], tot)
        return tot

    def cost(self, m):
        tot = np.zeros(m.shape[0])
        for i in range(m.shape[1]): tot = tot + m[:, i] * self.c[:, i]
        return tot


def _nan_max(worst, x):
    return np.where((x > worst) | (x != x), x, worst)


def _objective(P, members, points, errs):
    """group objective from per-output sample points (list of (k, L)) or errors (list of (k,)); NaN -> inf"""
    k, L = members.shape
    if P.budget_mode:
        obj = np.zeros(k)
        for e in errs: obj = _nan_max(obj, e)
    else:
        mx = np.zeros((k, L))
        for pt in points: mx = _nan_max(mx, pt)
        obj = np.zeros(k)
        for i in range(L): obj = obj + mx[:, i] * P.w[members[:, i]]
    return np.where(obj != obj, INF, obj)


def _sweep(P, members, levels, rounding):
    """the objective with every sample rounded one way (None, np.floor, np.ceil): (obj, feasible, passes)"""
    k = len(members)
    feasible, passes = np.ones(k, dtype=bool), np.ones(k, dtype=bool)
    points, errs = [], []
    for n, V in enumerate(levels):
        m = V.m if rounding is None else rounding(V.m)
        feasible &= V.finite
        if rounding is not None: feasible &= ~np.isnan(m).any(axis=1)
        var = V.variance(m)
        if P.budget_mode:
            passes &= V.cost(m) <= P.budget
            errs.append(np.sqrt(var))
        else:
            passes &= var <= P.eps2[n]
            points.append(m)
    return _objective(P, members, points, errs), feasible, passes


def bounds(m):
    """lb, ub and the position of each bound entry (get_feasible_integer_bounds, misc.py:141-167): entry j of the 2^L
    combinations rounds position pos[:, j]"""
    lb, ub = np.floor(m), np.ceil(m)
    idx = np.argsort(m, axis=1, kind="stable")
    ord2 = np.argsort(np.take_along_axis(lb, idx, axis=1), axis=1, kind="stable")
    pos = np.take_along_axis(idx, ord2[:, ::-1], axis=1)
    return lb, ub, pos


def _round_output(P, V, n, full):
    """k_mlmc_round for one output of the groups of V: (fval, combo, the chosen point per position)"""
    k, L = V.m.shape
    lb, ub, pos = bounds(V.m)
    fval, combo, point = np.full(k, INF), np.zeros(k, dtype=np.uint32), lb.copy()
    frac = np.take_along_axis(lb != ub, pos, axis=1)                    # per bound entry j
    nfrac = np.full(k, L) if full else frac.sum(axis=1)
    rows_all = np.arange(k)
    for nf in np.unique(nfrac):
        sel = rows_all[nfrac == nf]
        g = len(sel)
        Vs = object.__new__(_Level)
        Vs.v, Vs.c = V.v[sel], V.c[sel]
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
            cost, var = Vs.cost(pt), Vs.variance(pt)
            f = np.where(cost <= P.budget, var, INF) if P.budget_mode else np.where(var <= P.eps2[n], cost, INF)
            win = f < bf
            bf, bc = np.where(win, f, bf), np.where(win, c, bc)
            bp[win] = pt[win]
        fval[sel], combo[sel], point[sel] = bf, np.where(bf < INF, bc, 0).astype(np.uint32), bp
    return fval, combo, point


def _eval_size(P, masks, L, full):
    """every group of L models: dict of arrays (ok, obj, combos, lb, ub)"""
    k = len(masks)
    members = members_of(masks, L, P.nb)
    out = {"ok": np.zeros(k, dtype=bool), "obj": np.full(k, INF), "combos": np.zeros((k, P.n_out), dtype=np.uint32),
           "lb": np.full(k, INF), "ub": np.full(k, INF), "big": np.zeros(k, dtype=bool)}
    with np.errstate(all="ignore"):
        levels = [_Level(P, members, n) for n in range(P.n_out)]
        if P.continuous:
            out["obj"], out["ok"], _ = _sweep(P, members, levels, None)
            out["obj"] = np.where(out["ok"], out["obj"], INF)
            return out
        if L > MAX_ROUND:
            out["big"] = levels[0].finite.copy()
            return out
        down, up = (np.ceil, np.floor) if P.budget_mode else (np.floor, np.ceil)
        lb, ok, _ = _sweep(P, members, levels, down)
        ub, _, passes = _sweep(P, members, levels, up)
        out["ok"], out["lb"], out["ub"] = ok, np.where(ok, lb, INF), np.where(ok & passes, ub, INF)
        feasible, points, errs = ok.copy(), [], []
        for n, V in enumerate(levels):
            fval, out["combos"][:, n], point = _round_output(P, V, n, full)
            feasible &= fval < INF
            points.append(point)
            errs.append(np.sqrt(fval))
        out["obj"] = np.where(feasible, _objective(P, members, points, errs), INF)
    return out


def check_args(nb, n_out, flags, eps2, w, lv, adj, outputs_given=True):
    if nb < 0 or nb > MAX_CANDIDATES or n_out <= 0 or n_out > MAX_OUTPUTS: return ERR_ARG
    if w is None or lv is None or adj is None or not outputs_given: return ERR_ARG
    if not flags & BUDGET and eps2 is None: return ERR_ARG
    return RC_OK


class _Prob(object):
    pass


def search(nb, n_out, flags, budget, eps2, w, lv, adj, full=False, outputs_given=True):
    """bluest_mlmc_search: Result (rc, status, best_mask, best_combo, best_obj, facts)"""
    rc = check_args(nb, n_out, flags, eps2, w, lv, adj, outputs_given)
    if rc: return Result(rc)
    P = _Prob()
    P.nb, P.n_out, P.budget = nb, n_out, float(budget)
    P.budget_mode, P.continuous = bool(flags & BUDGET), bool(flags & CONTINUOUS)
    P.w = np.asarray(w, dtype=np.float64).reshape(nb + 1)
    P.lv = np.asarray(lv, dtype=np.float64).reshape(n_out, nb + 1, nb + 1)
    P.eps2 = None if eps2 is None else np.asarray(eps2, dtype=np.float64)
    groups = sorted(enumerate_groups(nb, adj), key=lambda m: order_key(m, nb))
    sizes = np.array([bin(m).count("1") + 1 for m in groups])
    masks = np.array(groups, dtype=np.uint32)
    F = {"groups": len(groups), "largest": int(sizes.max())}
    ev = {k: np.zeros((len(groups),) + s, dtype=t) for k, s, t in (("ok", (), bool), ("obj", (), float), ("lb", (), float),
                                                                  ("ub", (), float), ("big", (), bool),
                                                                  ("combos", (n_out,), np.uint32))}
    for L in np.unique(sizes)[::-1]:                          # the largest first: TOO_BIG is known before anything is rounded
        if L <= MAX_ROUND and ev["big"][sizes > MAX_ROUND].any(): break
        sel = np.flatnonzero(sizes == L)
        e = _eval_size(P, masks[sel], int(L), full)
        for k in ev: ev[k][sel] = e[k]
    if ev["big"].any():
        F["too_big"] = True
        return Result(RC_OK, TOO_BIG, None, None, None, F)
    obj = ev["obj"]
    F["feasible"] = int((obj < INF).sum())
    if not P.continuous:                                      # what the kernel's bounds would round
        U = float(ev["ub"].min())
        finite = ev["ok"] & np.isfinite(ev["lb"])
        hi0 = min(U, float(ev["lb"][finite].max())) if finite.any() else 0.0
        F["min_ub"], F["candidates"] = U, int((ev["ok"] & (ev["lb"] <= hi0)).sum())
        F["bounds_hold"] = bool(np.all((ev["lb"] <= obj) | ~ev["ok"]) and np.all((obj <= ev["ub"]) | ~ev["ok"]))
        same = np.unique(ev["lb"][ev["ok"] & (ev["lb"] <= hi0)], return_counts=True)[1]
        F["most_sharing_one_lb"] = int(same.max()) if same.size else 0
    best = int(np.argmin(obj))                                # first minimum: ties go to the earlier group
    if not obj[best] < INF:
        return Result(RC_OK, NONE, 0xffffffff, np.zeros(n_out, dtype=np.uint32), INF, F)
    F["winner_size"], F["highest_bit"] = int(sizes[best]), int(masks[best]).bit_length() - 1
    F["tied_masks"] = [int(m) for m in masks[obj == obj[best]] if int(m) != int(masks[best])]
    F["objectives"] = dict(zip((int(m) for m in masks), obj.tolist())) if len(masks) <= 4096 else None
    return Result(RC_OK, OK, int(masks[best]), ev["combos"][best].copy(), float(obj[best]), F)


# ------------------------------------------------------------------------------------------------------
# around the kernel: what MLMCMixin.setup_mlmc does before and after it (blue_models.py:642-741)
# ------------------------------------------------------------------------------------------------------
def inputs_from_covariances(Cs, w, dV=None, budget=None, eps=None, continuous_relaxation=False):
    """the kernel's arguments for the covariances Cs (one per output; an infinite or zero entry: the pair is never coupled),
    the mlmc_variances dV and the costs w: dict of search()'s arguments, plus `idx` (the model at each position)"""
    Cs = [np.asarray(C, dtype=np.float64) for C in Cs]
    w = np.asarray(w, dtype=np.float64)
    M, n_out = len(w), len(Cs)
    dV = [np.full((M, M), np.nan)] * n_out if dV is None else dV
    linked = np.ones((M, M), dtype=bool)
    for C in Cs:
        coupled = ~np.isinf(C) & (C != 0.0)
        linked &= coupled & coupled.T
    idx = np.argsort(w)[::-1][int((w > w[0]).sum()):]
    assert idx[0] == 0
    nb = len(idx) - 1
    lv = np.full((n_out, nb + 1, nb + 1), np.nan)
    for n, C in enumerate(Cs):
        for p in range(nb + 1):
            lv[n, p, p] = C[idx[p], idx[p]]
            for q in range(p + 1, nb + 1):
                a, b = idx[p], idx[q]
                check = dV[n][min(a, b), max(a, b)]
                lv[n, p, q] = check if np.isfinite(check) else C[a, a] + (C[b, b] - 2 * C[a, b])
    adj = np.array([sum(1 << q for q in range(nb + 1) if q != p and linked[idx[p], idx[q]]) for p in range(nb + 1)], dtype=np.uint32)
    flags = (BUDGET if budget is not None else 0) | (CONTINUOUS if continuous_relaxation else 0)
    if budget is None and np.isscalar(eps): eps = [eps] * n_out
    return dict(nb=nb, n_out=n_out, flags=flags, budget=float(budget or 0.0),
                eps2=None if budget is not None else np.array([e**2 for e in eps]), w=w[idx].copy(), lv=lv, adj=adj), idx


def host_finish(args, idx, mask, combo):
    """{"models", "samples", "errors", "total_cost"} as setup_mlmc reports them for the kernel's answer (blue_models.py:725-734)"""
    P = _Prob()
    P.nb, P.n_out, P.budget, P.budget_mode = args["nb"], args["n_out"], args["budget"], bool(args["flags"] & BUDGET)
    P.w, P.lv, P.eps2 = args["w"], args["lv"], args["eps2"]
    L = bin(mask).count("1") + 1
    members = members_of([mask], L, P.nb)
    with np.errstate(all="ignore"):
        levels = [_Level(P, members, n) for n in range(P.n_out)]
    per_output = []
    for n, V in enumerate(levels):
        m = V.m[0]
        if not args["flags"] & CONTINUOUS:
            lb, ub, pos = bounds(V.m)
            m = lb[0].copy()
            for j in range(L):
                if (int(combo[n]) >> j) & 1: m[pos[0, j]] = ub[0, pos[0, j]]
            m = m.astype(np.int64)
        per_output.append(m)
    samples = np.max(np.vstack(per_output), axis=0)
    wm = P.w[members[0]]
    cost = samples @ wm
    if P.budget_mode:
        samples = np.floor(samples - (max(cost - P.budget, 0) / (wm @ wm)) * wm).astype(int)
        samples[0] = max(samples[0], 1)
        cost = samples @ wm
    errs = [np.sqrt(sum(V.v[0][samples > 0] / samples[samples > 0])) for V in levels]
    return {"models": [int(idx[p]) for p in members[0]], "samples": samples, "errors": errs, "total_cost": cost}

"""
The device-resident SPG state machine (csrc/spg.hip, csrc/spg_state.hpp) restated launch by launch in plain numpy.

One pure function per launch.  Each takes the 256-double state and the vectors the launch reads, and returns a `Launch`:
what the launch must leave in every word it may write, and for every continuous word the absolute error a float64
evaluation of the same formula may have.  Whatever a float64 kernel computes in float64 is computed here in `wide`
(np.longdouble by default; np.float64 turns the restatement into a model of the device arithmetic, which the CPU tests use to
count how many Armijo tests of a run are too close to call).

Error model (EPS = 2^-52; one correctly rounded operation errs by at most EPS/2 relative, every bound below counts whole
EPS per operation, so each carries a factor of about 2 of slack and nothing else):
  dot product   sum_i a_i b_i over n terms, any summation order: n EPS sum_i |a_i b_i| (+ what the inputs carry).  Absolute,
                not relative to the result: s.y cancels.
  projection    tau solves sum_i s_i max(r_i - tau, 0) = z.  It is a weighted mean of the active r_i (shifted by their
                maximum) minus z / s0, so it moves by at most the largest perturbation of an r_i: EPS max|r| for the rounding
                of r_i = q_i - lambda g_i, twice for the shift and the mean.  Below that the existing projection tests
                (tests/test_gpu_parity.py) hold p to 1e-12 z; the bound is the larger of the two.
Discrete words (flags, counters, the history slot) carry no bound: they are equal or the kernel is wrong.
"""
from fractions import Fraction

import numpy as np

EPS = 2.0 ** -52
LD = np.longdouble

# state layout (csrc/spg_state.hpp)
F, FNEW, LAMBDA, ALPHA, GD, DMAX, TAU, NPOS, ACCEPT, FAIL, DONE, IT, COUNT, NORM, P, LMIN, LMAX, HLEN, SDOTS, SDOTY, FTRIAL = range(21)
EPS_W, PENDING, MAXFEV, GPSTATS, TICKET, GDPARTS, GDPARTS_N, THETA = 21, 22, 23, 24, 28, 29, 30, 31
HIST, COEF, S, STATE_DOUBLES = 32, 64, 128, 256
EVAL_OK = 0
ARMIJO = 1.0e-4
# words a direction launch may use as private scratch (pointer to the g.d partials, warm start of the threshold search):
# they are compared by no test of a direction launch, and must be bit-identical across every other launch
SCRATCH = (GDPARTS, THETA)


class Launch(object):
    """state: float64[256] expected state; bound: float64[256] absolute bounds (0 = exact); vec / vbound: name -> expected
    vector / bound for every vector the launch writes (absent = untouched); enable: expected gate or None (untouched);
    extra: figures of the launch that live in no state word (g.d of a multi-workgroup direction, the Armijo margin, ...)"""

    def __init__(self, state):
        self.state = np.array(state, dtype=np.float64)
        self.bound = np.zeros(STATE_DOUBLES)
        self.written = np.zeros(STATE_DOUBLES, dtype=bool)
        self.vec, self.vbound = {}, {}
        self.enable = None
        self.extra = {}

    def put(self, word, value, bound=0.0):
        self.state[word] = np.float64(value)
        self.bound[word] = float(bound)
        self.written[word] = True


def idle(state):
    return state[DONE] != 0.0 or state[FAIL] != 0.0


def fma_exact(a, x, y):
    """fma(a, x_i, y_i) rounded once, element by element.  The 80-bit evaluation a*x + y carries two roundings of 2^-64 relative;
    rounded to float64 it is the correctly rounded exact value unless it lies within that error of a float64 rounding midpoint.
    Those few entries (about one in a thousand) are redone in exact rational arithmetic (float() of a Fraction rounds correctly)."""
    x, y = np.asarray(x, dtype=np.float64), np.asarray(y, dtype=np.float64)
    assert np.finfo(LD).nmant >= 63, "needs an extended-precision long double"
    al = LD(float(a))
    prod = al * x.astype(LD)
    v = prod + y.astype(LD)
    r = v.astype(np.float64)
    err = LD(2.0) ** -62 * (np.abs(prod) + np.abs(v))
    rl = r.astype(LD)
    mid_lo = (rl + np.nextafter(r, -np.inf).astype(LD)) / 2
    mid_hi = (rl + np.nextafter(r, np.inf).astype(LD)) / 2
    sus = (np.abs(v - mid_lo) <= err) | (np.abs(v - mid_hi) <= err) | ~np.isfinite(r) | (np.abs(r) < 1e-290)
    fa = Fraction(float(a))
    for i in np.flatnonzero(sus):
        r[i] = float(fa * Fraction(float(x[i])) + Fraction(float(y[i])))
    return r


def trial_point(alpha, x, d, scale):
    xnew = fma_exact(alpha, d, x)
    return xnew, scale * xnew             # one rounded product in float64, as the kernel's


# ---- projection ---------------------------------------------------------------------------------------------------
def project(x, g, lam, z, floor, wide=LD):
    """P_s(x - lam s g) with s = max(x, floor) (1 when floor == 0), in the kernels' variables r_i = x_i/s_i - lam g_i:
    p_i = s_i max(r_i - tau, 0).  The threshold search is oracle.weighted_simplex_projection's sort, in `wide`.
    Returns p, d = p - x, (g.d, max|d|, tau - max r, #positive) and their bounds."""
    xw, gw = np.asarray(x, dtype=wide), np.asarray(g, dtype=wide)
    lam, z, floor = wide(lam), wide(z), wide(floor)
    if floor > 0:
        s = np.maximum(xw, floor)
        q = np.where(xw >= floor, wide(1.0), xw / floor)
    else:
        s = np.ones(len(xw), dtype=wide)
        q = xw
    r = q - lam * gw
    rmax = r.max()
    rr = r - rmax
    order = np.argsort(-rr, kind="stable")
    rs, ss = rr[order], s[order]
    taus = (np.cumsum(ss * rs) - z) / np.cumsum(ss)
    k = np.nonzero(rs > taus)[0][-1]
    tau = taus[k]
    p = s * np.maximum(rr - tau, wide(0.0))
    d = p - xw
    # threshold: 4 EPS max|r| (rounding of r_i, of the shift by max r, of the weighted mean; see the module docstring), or
    # what the existing projection tests demand of p at the largest weight, whichever is larger
    rabs = float(np.abs(r).max())
    btau = max(1e-12 * float(z) / float(s.max()), 4.0 * EPS * rabs)
    bp = s.astype(np.float64) * btau
    bd = bp + EPS * np.abs(d).astype(np.float64)                      # d = p - x: one more rounding
    terms = np.abs(gw * d).astype(np.float64)
    # g.d: a dot product of L terms (L EPS sum|g_i d_i|) whose second factor carries bd
    bgd = len(xw) * EPS * float(terms.sum()) + float((np.abs(gw).astype(np.float64) * bd).sum())
    npos_sure = int(((rr - tau) > btau).sum())
    npos_maybe = int(((rr - tau) > -btau).sum())
    stats = (float((gw * d).sum()), float(np.abs(d).max()), float(tau), int((p > 0).sum()))
    bounds = (bgd, float(bd.max()), btau + EPS * rabs, (npos_sure, npos_maybe))
    return p.astype(np.float64), d.astype(np.float64), bp, bd, stats, bounds


def _put_stats(out, base, stats, bounds):
    out.put(base + 0, stats[0], bounds[0])
    out.put(base + 1, stats[1], bounds[1])
    out.put(base + 2, stats[2], bounds[2])
    out.put(base + 3, stats[3], 0.0)
    out.extra["npos_range"] = bounds[3]                  # entries within the bound of the threshold may fall either side


def direction(state, x, g, d, scale, z, floor, workgroups=0, trial=True, wide=LD):
    """bluest_spg_direction.  workgroups = 0: a launch that folds its statistics itself (k_simplex, the multi-launch chain):
    GD, DMAX, TAU, NPOS are written and GDPARTS_N = 0.  workgroups > 0: the single-launch k_proj_fused with that many
    workgroups, which leaves only per-workgroup partials of g.d (GDPARTS_N = workgroups; DMAX, TAU, NPOS untouched); the
    folded g.d and its bound are in extra["gd"], extra["gd_bound"] for the decision that consumes them."""
    out = Launch(state)
    if idle(state):
        if trial:
            out.enable = 0
        return out
    if state[PENDING] != 0.0:
        # the line search of this iteration goes on: no new direction, the next trial point instead
        if trial:
            xnew, m = trial_point(state[ALPHA], x, d, scale)
            out.vec["xnew"], out.vec["m"] = xnew, m
            out.vbound["xnew"] = out.vbound["m"] = 0.0                # bit for bit
            out.enable = 1
        return out
    p, dd, bp, bd, stats, bounds = project(x, g, state[LAMBDA], z, floor, wide)
    out.vec["d"], out.vbound["d"] = dd, bd
    if trial:
        # alpha = 1: xnew = p, m = scale * p (one product: EPS |m| on top of scale * bp)
        out.vec["xnew"], out.vbound["xnew"] = p, bp
        out.vec["m"] = scale * p
        out.vbound["m"] = np.abs(scale) * bp + EPS * np.abs(out.vec["m"])
        out.enable = 1
    if workgroups > 0:
        out.put(GDPARTS_N, workgroups)
        out.extra["gd"], out.extra["gd_bound"] = stats[0], bounds[0]
    else:
        _put_stats(out, GD, stats, bounds)
        out.put(GDPARTS_N, 0.0)
    return out


def converged(state, x, g, z, floor, wide=LD):
    """bluest_spg_converged: the projection with lambda = 1 into GPSTATS, DONE iff max|gp| <= EPS.  extra["done_margin"] is how
    far max|gp| is from EPS beyond its bound (not positive: either value of DONE is right)."""
    out = Launch(state)
    if idle(state):
        return out
    _, _, _, _, stats, bounds = project(x, g, 1.0, z, floor, wide)
    _put_stats(out, GPSTATS, stats, bounds)
    done = stats[1] <= state[EPS_W]
    out.extra["done_margin"] = abs(stats[1] - state[EPS_W]) - bounds[1]
    if done:
        out.put(DONE, 1.0)
    out.extra["done"] = bool(done)
    return out


def trial(state, x, d, scale):
    """k_spg_trial: the next trial point, unless the run is over or this iteration already accepted; the gate says which"""
    out = Launch(state)
    run = not idle(state) and state[ACCEPT] == 0.0
    out.enable = 1 if run else 0
    if run:
        out.vec["xnew"], out.vec["m"] = trial_point(state[ALPHA], x, d, scale)
        out.vbound["xnew"] = out.vbound["m"] = 0.0
    return out


# ---- line-search decision -----------------------------------------------------------------------------------------
def objective(state, var, status, n_out, wide=LD):
    """F = ||V_o / s_o||_p / norm and dF/dV_o / norm, with bounds.  Any status other than OK, or a ratio that is not finite,
    gives F = inf."""
    V = np.asarray(var[:n_out], dtype=wide)
    so = np.asarray(state[S:S + n_out], dtype=wide)
    with np.errstate(all="ignore"):
        r = V / so
    if (np.asarray(status[:n_out]) != EVAL_OK).any() or not np.isfinite(r.astype(np.float64)).all():
        return np.inf, 0.0, None, None
    norm, p = wide(state[NORM]), float(state[P])
    rmax = r.max()
    if np.isinf(p) or n_out == 1:
        omax = int(np.argmax(r))                                       # the first maximal output wins ties
        coef = np.zeros(n_out, dtype=wide)
        coef[omax] = wide(1.0) / so[omax] / norm
        Fv = rmax / norm
        # two divisions (V/s, /norm); the coefficient: 1/s, /norm
        return float(Fv), 2.0 * EPS * abs(float(Fv)), coef.astype(np.float64), 2.0 * EPS * np.abs(coef).astype(np.float64)
    q = r / rmax
    tq = q ** wide(p - 1.0)
    tsum = (tq * q).sum()
    root = tsum ** (wide(1.0) / wide(p))
    Fv = rmax * root / norm
    coef = tq * (root / tsum) / so / norm
    # q = (V/s)/rmax: two divisions, 2 EPS relative.  pow(q, p-1) amplifies that (p-1) times and adds its own error (2 EPS for a
    # pow good to about one ulp): rel(tq) = (2 (p-1) + 2) EPS.  The sum has positive terms tq*q, so relative errors carry over:
    # rel(tsum) = rel(tq) + 2 EPS (q, the product) + n_out EPS (summation).  root = pow(tsum, 1/p) divides that by p, plus
    # 2 EPS for the pow, plus the rounding of 1/p seen through t^(1/p): ln(tsum) EPS / p <= ln(64) EPS / p.
    rel_tq = (2.0 * (p - 1.0) + 2.0) * EPS
    rel_tsum = rel_tq + (2.0 + n_out) * EPS
    rel_root = rel_tsum / p + 2.0 * EPS + np.log(64.0) * EPS / p
    bF = (rel_root + 2.0 * EPS) * abs(float(Fv))                       # rmax * root, / norm
    bcoef = (rel_tq + rel_root + rel_tsum + 4.0 * EPS) * np.abs(coef).astype(np.float64) + 1e-300   # root/tsum, *, /s, /norm
    return float(Fv), bF, coef.astype(np.float64), bcoef


def decide(state, var, status, n_out, last_slot, gd_parts=None, force_accept=None, wide=LD):
    """spg_decide_wave.  gd_parts: the per-workgroup partials of g.d when GDPARTS_N > 0 (the kernel then ignores the GD word).
    force_accept: take that branch whatever the Armijo test says (for a step whose margin is not positive the caller reads
    the branch off the device and checks the rest of the state against it).
    extra: F, F_bound, threshold, margin (|F - threshold| minus the bounds of both sides), accept; alpha_alt: the other value
    the interpolation safeguard could yield when the interpolated step is within its bound of 0.1 or 0.9 alpha."""
    out = Launch(state)
    st = state
    if idle(st) or st[ACCEPT] != 0.0:
        if last_slot:
            out.enable = 1 if (not idle(st) and st[ACCEPT] != 0.0) else 0
        out.extra["early"] = True
        return out
    Fv, bF, coef, bcoef = objective(st, var, status, n_out, wide)
    H = int(st[HLEN])
    fmax = -np.inf
    for h in range(H):
        fmax = fmax if fmax > st[HIST + h] else st[HIST + h]
    if int(st[GDPARTS_N]) > 0:
        parts = np.asarray(gd_parts, dtype=wide)
        gd = parts.sum()
        bgd = len(parts) * EPS * float(np.abs(parts).sum())            # fixed-order fold of <= 64 partials
    else:
        gd, bgd = wide(st[GD]), 0.0
    alpha, f = wide(st[ALPHA]), wide(st[F])
    step = wide(ARMIJO) * alpha * gd
    thr = wide(fmax) + step
    # threshold: two products and a sum (3 EPS |step| + EPS |thr|), plus what g.d carries
    bthr = 3.0 * EPS * abs(float(step)) + EPS * abs(float(thr)) + ARMIJO * float(alpha) * bgd
    margin = abs(Fv - float(thr)) - bF - bthr if np.isfinite(Fv) else np.inf
    accept = bool(Fv <= thr)
    out.extra.update(F=Fv, F_bound=bF, threshold=float(thr), margin=margin, accept=accept, early=False, gd=float(gd), gd_bound=bgd)
    if force_accept is not None:
        accept = bool(force_accept)
    out.put(COUNT, st[COUNT] + 1.0)
    out.put(FTRIAL, Fv, bF)
    if accept:
        for o in range(n_out):
            out.put(COEF + o, coef[o], bcoef[o])
        out.put(ACCEPT, 1.0)
        out.put(FNEW, Fv, bF)
        out.put(PENDING, 0.0)
    else:
        a = alpha
        balpha = 0.0
        if a <= 0.1:
            a = a * wide(0.5)                                          # exact
        else:
            with np.errstate(all="ignore"):
                num = wide(-0.5) * (a * a) * gd
                den = wide(Fv) - f - a * gd
                at = num / den
            half = wide(0.5) * a
            if np.isfinite(float(at)):
                # numerator: three products (3 EPS) and the error of g.d; denominator F - f - a gd: bF, two sums and a product
                # (EPS (|F| + |f| + 2 |a gd|)), a bgd; the quotient: rel(num) + b(den)/|den| + EPS
                bden = bF + EPS * (abs(Fv) + abs(float(f)) + 2.0 * abs(float(a * gd))) + float(a) * bgd
                rel = 3.0 * EPS + (bgd / abs(float(gd)) if gd != 0 else 0.0) + bden / abs(float(den)) + EPS
                bat = rel * abs(float(at))
                inside = (at >= 0.1) and not (at > wide(0.9) * a)
                near = min(abs(float(at) - 0.1), abs(float(at) - 0.9 * float(a))) <= bat + EPS * float(a)
                if near:
                    out.extra["alpha_alt"] = float(at if not inside else half)
                    out.extra["alpha_alt_bound"] = bat if not inside else 0.0
                a, balpha = (at, bat) if inside else (half, 0.0)
            else:
                a = half                                               # F = inf gives at = -0, NaN fails every comparison
        out.put(ALPHA, a, balpha)
        if last_slot:
            maxfev = st[MAXFEV]
            dead = (not (a >= 1.0e-300)) or (maxfev > 0.0 and st[COUNT] + 1.0 >= maxfev)
            out.put(FAIL if dead else PENDING, 1.0)
    if last_slot:
        out.enable = 1 if accept else 0
    return out


# ---- accepted step --------------------------------------------------------------------------------------------------
def combine(state, grads, maps, scale, L, n_out, wide=LD):
    """gnew_j = scale_j sum_o COEF_o grad_o[local_o(j)] (maps[o]: global index of every local group of output o), and its
    bound: n_out fma steps and one product, (n_out + 1) EPS scale_j sum_o |COEF_o grad_o|"""
    acc = np.zeros(L, dtype=wide)
    mag = np.zeros(L, dtype=np.float64)
    for o in range(n_out):
        term = wide(state[COEF + o]) * np.asarray(grads[o], dtype=wide)
        acc[maps[o]] += term
        mag[maps[o]] += np.abs(term).astype(np.float64)
    sw = np.asarray(scale, dtype=wide)
    return (acc * sw).astype(np.float64), (n_out + 1) * EPS * np.abs(scale) * mag


def update(state, x, g, xnew, gnew, floor, gnew_bound=None, wide=LD):
    """k_spg_update_a + spg_update_tail (and the tails of k_spg_update_a_fused / k_spg_finish_small, whose gnew comes from
    combine() with gnew_bound).  A no-op unless ACCEPT is set and the run is live."""
    out = Launch(state)
    if idle(state) or state[ACCEPT] == 0.0:
        return out
    xw, gw, xn, gn = (np.asarray(a, dtype=wide) for a in (x, g, xnew, gnew))
    bgn = np.zeros(len(xw)) if gnew_bound is None else np.asarray(gnew_bound, dtype=np.float64)
    n = len(xw)
    s = xn - xw
    y = gn - gw
    sabs = np.abs(s).astype(np.float64)
    if floor > 0:
        t = s * s / np.maximum(xw, wide(floor))
    else:
        t = s * s
    sdots, sdoty = t.sum(), (s * y).sum()
    # s^T D^-1 s: every term is s_i (rounded difference, twice), a product and a division: 4 EPS relative, then a sum of n
    # non-negative terms: (n + 4) EPS sum t_i
    bs = (n + 4.0) * EPS * float(t.sum())
    # s.y: n EPS sum|s_i y_i| for the summation; s_i and y_i are rounded differences (2 EPS sum|s_i y_i|); y_i also carries
    # the error of gnew_i.  Absolute: the sum cancels.
    by = (n + 2.0) * EPS * float(np.abs(s * y).sum()) + float((sabs * bgn).sum())
    out.vec["x"], out.vbound["x"] = np.array(xnew, dtype=np.float64), 0.0
    out.vec["g"], out.vbound["g"] = np.array(gnew, dtype=np.float64), bgn if gnew_bound is not None else 0.0
    out.put(SDOTS, sdots, bs)
    out.put(SDOTY, sdoty, by)
    lmin, lmax = state[LMIN], state[LMAX]
    sure = abs(float(sdoty)) > by                                      # the sign of s.y is beyond its bound
    out.extra["sdoty_sign_sure"] = sure
    if sdoty <= 0:
        lam, blam = lmax, 0.0
    else:
        ratio = float(sdots / sdoty)
        lam = min(lmax, max(lmin, ratio))
        # quotient: relative errors add, plus the division; the clamp is 1-Lipschitz, so the bound survives it
        blam = ratio * (bs / float(sdots) + by / float(sdoty) + EPS) if sdots > 0 else 0.0
    out.put(LAMBDA, lam, blam if sure else np.inf)
    it = state[IT] + 1.0
    out.put(IT, it)
    out.put(F, state[FNEW])
    out.put(HIST + int(it) % int(state[HLEN]), state[FNEW])
    out.extra["hist_slot"] = int(it) % int(state[HLEN])
    out.put(ALPHA, 1.0)
    out.put(ACCEPT, 0.0)
    return out


# ---- the whole machine (CPU only: anchors the restatement against recorded runs, counts undecidable steps) ---------
def initial_state(norm, gpmax, n_out, s_norm, p, H, lmin, lmax, eps, maxfev, f0=1.0):
    """what DeviceSpg.run uploads before the first window (it normalises by the first objective: norm = F0, f0 = 1)"""
    h = np.zeros(STATE_DOUBLES)
    h[F] = f0
    h[LAMBDA] = min(lmax, max(lmin, 1.0 / gpmax)) if gpmax > 1e-15 else 0.0
    h[ALPHA] = 1.0
    h[COUNT] = 1.0
    h[NORM], h[P], h[LMIN], h[LMAX], h[HLEN] = norm, p, lmin, lmax, H
    h[HIST:HIST + 16] = -np.inf
    h[HIST] = f0
    h[S:S + n_out] = s_norm
    h[EPS_W] = eps
    h[MAXFEV] = float(maxfev)
    h[GPSTATS + 1] = gpmax
    return h


def apply(state, x, g, d, xnew, m, launch):
    """the arrays after a launch: its expected values where it writes, the old ones elsewhere"""
    v = {"x": x, "g": g, "d": d, "xnew": xnew, "m": m}
    v.update(launch.vec)
    return launch.state.copy(), v["x"], v["g"], v["d"], v["xnew"], v["m"]


def run_machine(evaluate, x0, scale, s_norm, p=np.inf, floor=0.0, H=10, lmin=1e-30, lmax=1e30, eps=1e-9, maxit=60,
                maxfev=10 ** 5, slots=1, wide=LD, on_eval=None, normalise=True):
    """the launch sequence of bluest_spg_window with one iteration per window and the convergence projection after each, driven
    by evaluate(m) -> (var[n_out], status[n_out], grads: list of per-output gradients dV_o/dm over ALL groups, or a
    callable that returns it: only the accepted trial's gradient is ever used).
    normalise=False keeps NORM = 1: the reference's own iteration, which takes its first spectral step from the gradient of the
    objective as it is.  Returns the final state, x, and a log of the decisions (margin, accept)."""
    n_out = len(s_norm)
    L = len(x0)
    maps = [np.arange(L)] * n_out
    x = project(np.asarray(x0, dtype=np.float64), np.zeros(L), 0.0, 1.0, 0.0, wide)[0]
    var, status, grads = evaluate(scale * x)
    if on_eval:
        on_eval(var)
    st0 = np.zeros(STATE_DOUBLES)
    st0[NORM], st0[P] = 1.0, p
    st0[S:S + n_out] = s_norm
    F0, _, coef0, _ = objective(st0, var, status, n_out, wide)
    norm = F0 if normalise else 1.0
    st0[COEF:COEF + n_out] = coef0 / norm
    g = combine(st0, grads() if callable(grads) else grads, maps, scale, L, n_out, wide)[0]
    gpmax = project(x, g, 1.0, 1.0, floor, wide)[4][1]
    state = initial_state(norm, gpmax, n_out, s_norm, p, H, lmin, lmax, eps, maxfev, f0=F0 / norm)
    if gpmax <= eps:
        state[DONE] = 1.0
    d, xnew, m = np.zeros(L), x.copy(), scale * x
    log = []
    enable = 1
    cache = None
    for _ in range(50 * maxit):                                        # a step that ends PENDING completes no iteration
        if idle(state) or state[IT] >= maxit:
            break
        la = direction(state, x, g, d, scale, 1.0, floor, 0, True, wide)
        state, x, g, d, xnew, m = apply(state, x, g, d, xnew, m, la)
        enable = la.enable
        for t in range(slots):
            last = 1 if t == slots - 1 else 0
            if t > 0:
                la = trial(state, x, d, scale)
                state, x, g, d, xnew, m = apply(state, x, g, d, xnew, m, la)
                enable = la.enable
            if enable:
                var, status, grads = evaluate(m)
                cache = grads
                if on_eval and not (idle(state) or state[ACCEPT] != 0.0):
                    on_eval(var)
            la = decide(state, var, status, n_out, last, wide=wide)
            if not la.extra["early"]:
                log.append((la.extra["margin"], la.extra["accept"]))
            state = la.state.copy()
            if la.enable is not None:
                enable = la.enable
        if enable:
            # the gradient of the accepted trial point: the last evaluation that ran is the accepted one (later slots are gated off)
            cache = cache() if callable(cache) else cache
            gnew, _ = combine(state, cache, maps, scale, L, n_out, wide)
            la = update(state, x, g, xnew, gnew, floor, wide=wide)
            state, x, g, d, xnew, m = apply(state, x, g, d, xnew, m, la)
        la = converged(state, x, g, 1.0, floor, wide)
        state = la.state.copy()
    return state, x, log

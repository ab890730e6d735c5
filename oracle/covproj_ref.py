"""
The covariance projection kernel (csrc/covproj.hip: bluest_cov_project, C-ABI Part 8) restated in numpy at the kernel's own
interface, in np.longdouble (64-bit mantissa).  Nothing of bluest_amd is imported.

  proj_ld(X, thr, lower_only)   V max(l, thr) V^T by cyclic Jacobi in longdouble, with the bound of what the kernel's float64
                                Jacobi and reassembly may differ from it
  step_ld(...)                  ONE SPG iteration as a pure function of (x, g, lambda, f, history ring, count): the new state,
                                next to every value the bound of what float64 rounding in the kernel can move, and the margin
                                of every decision taken
  run_ld(C, mask, params)       the start and the loop, ending as the kernel ends, with the kernel's `info`, and the trace

What the kernel computes bit for bit from values it returns is restated in float64 with the same operations (W = m * m,
Cm, g = am(x - Cm, W), 1 / gpmax): those carry no bound.  Everything that goes through a sum or an eigendecomposition is
computed in longdouble and carries one.

Bounds (u = 2^-53, N = M * M).  None is fitted to the kernel's output.

  Projection.  The kernel's Jacobi applies, per step of a sweep, Mp/2 disjoint rotations from both sides (Mp = M padded to
  even, Mp - 1 steps per sweep, at most MAX_SWEEPS sweeps).  A rotation (c, s) computed in floating point and applied to a
  pair of rows is an exactly orthogonal rotation applied to a pair perturbed by at most 6u in norm (Higham, Accuracy and
  Stability, Lemma 19.7/19.8 with gamma_6); both sides of one step, with the slack of the second-order terms: 16u ||A||_F.
  So the computed diagonal and V are the exact eigendecomposition (Vt, lt) of A + E, ||E||_F <= 16u * steps * ||A||_F, and
  the computed V is within 16u * steps * sqrt(M) of Vt in the Frobenius norm.  The eigenvalue clip is the metric
  projection onto a closed convex set: ||proj(A + E) - proj(A)||_F <= ||E||_F, whatever the spectrum -- no gap enters.
  V - Vt enters the reassembly V diag(l) V^T twice, each time scaled by ||clip(l)||_2 <= ||A||_F + thr.  Together
      3 * 16u * MAX_SWEEPS * (Mp - 1) * (||A||_F + thr sqrt(M))         (the term K_J),
  plus the entries left above zero, M * JACOBI_TOL * ||A||_F, plus u ||A||_F for the symmetrisation, plus the rounding of
  the reassembly itself, a sum of M products of three factors: (M + 2) u * sum_k |V_ik| |l_k| |V_jk|, per entry.

  A sum of n float64 terms in any order: (n - 1) u * sum |terms| (first order; every bound here is taken with a factor
  1 + 1e-6 for the second order).
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53
OK, MAXIT, MAXFEV, NONFINITE, NOEIG = 0, 1, 2, 3, 4
RC_OK, ERR_ARG = 0, 1
MAX_MODELS, MAX_OUTPUTS, MAX_HISTORY = 64, 1024, 64
MAX_SWEEPS, JACOBI_TOL = 40, 1e-18              # the kernel's sweep budget and rotation threshold
GAMMA, SIGMA_MIN, SIGMA_MAX = 1.0e-4, 0.1, 0.9
MASK_USED, W_USED = 1.0e-14, 1.0e-15            # |m| < 1e-14: entry unknown (C zeroed); |m^2| < 1e-15: entry weighs nothing
SLACK = 1.0 + 1e-6
LD_SWEEPS = 60

default_params = {"spd_threshold": 5.0e-14, "eps": 1.0e-10, "lmbda_min": 1e-30, "lmbda_max": 1e30, "maxit": 10000,
                  "max_fevals": 10000 ** 2, "hlength": 10}


def jacobi_ld(A):
    """(l, V, sweeps): cyclic-by-row Jacobi on a symmetric longdouble matrix until sum_{i != j} a_ij^2 <= (1e-30 ||A||_F)^2"""
    A = np.array(A, dtype=LD)
    M = A.shape[0]
    V = np.eye(M, dtype=LD)
    fro2 = (A * A).sum()
    one, two = LD(1), LD(2)
    for sweep in range(LD_SWEEPS + 1):
        off2 = sum((A[i, :i] ** 2).sum() + (A[i, i + 1:] ** 2).sum() for i in range(M))     # directly, not fro2 - diag2
        if off2 <= LD(1e-60) * fro2:
            return A.diagonal().copy(), V, sweep
        assert sweep < LD_SWEEPS, "the longdouble Jacobi did not converge"
        for p in range(M - 1):
            for q in range(p + 1, M):
                apq = A[p, q]
                if apq == 0:
                    continue
                tau = (A[q, q] - A[p, p]) / (two * apq)
                t = (one if tau >= 0 else -one) / (abs(tau) + np.sqrt(one + tau * tau))
                c = one / np.sqrt(one + t * t)
                s = t * c
                rp, rq = A[p].copy(), A[q].copy()
                A[p] = c * rp - s * rq
                A[q] = s * rp + c * rq
                cp, cq = A[:, p].copy(), A[:, q].copy()
                A[:, p] = c * cp - s * cq
                A[:, q] = s * cp + c * cq
                A[p, q] = A[q, p] = 0
                vp, vq = V[:, p].copy(), V[:, q].copy()
                V[:, p] = c * vp - s * vq
                V[:, q] = s * vp + c * vq


def k_jacobi(M):
    """the constant of the projection bound that multiplies u (||A||_F + thr sqrt(M)); see the module docstring"""
    Mp = M + (M & 1)
    return 3.0 * 16.0 * MAX_SWEEPS * max(Mp - 1, 1) + M * JACOBI_TOL / U + 1.0


def proj_ld(X, thr, lower_only=False):
    """(P, bound): P = V max(l, thr) V^T of the symmetric part of X (or of the matrix its lower triangle gives), longdouble;
    bound[i, j] >= |kernel's float64 proj - P|[i, j]"""
    X = np.array(X, dtype=LD)
    M = X.shape[0]
    A = np.tril(X) + np.tril(X, -1).T if lower_only else (X + X.T) / LD(2)
    l, V, _ = jacobi_ld(A)
    thr = LD(thr)
    l = np.where(l < thr, thr, l)
    P = (V * l) @ V.T
    P = (P + P.T) / LD(2)
    fro = np.sqrt((A * A).sum())
    S = (np.abs(V) * np.abs(l)) @ np.abs(V).T
    bound = SLACK * U * (k_jacobi(M) * (fro + abs(thr) * np.sqrt(LD(M))) + (M + 2) * S)
    return P, bound


def prepare(C, mask):
    """(Cm, W, unknown, bad) as the kernel's first loop forms them, float64 bit for bit"""
    C = np.asarray(C, dtype=np.float64)
    m = np.asarray(mask, dtype=np.float64)
    W = m * m
    used = ~(np.abs(m) < MASK_USED)
    Cm = np.where(used, C, 0.0)
    bad = bool((~np.isfinite(m)).any() or (used & ~np.isfinite(C)).any())
    return Cm, W, bool((~used).any()), bad


def am64(v, W):
    """am(v, w) of the kernel in float64: zero where |w| < 1e-15, v * w elsewhere"""
    with np.errstate(invalid="ignore", over="ignore"):
        return np.where(np.abs(W) < W_USED, 0.0, v * W)


def grad64(x, Cm, W):
    """g = am(x - Cm, W): float64, the kernel's two operations, so bit-equal to the kernel's g for the same x"""
    return am64(np.asarray(x, dtype=np.float64) - Cm, W)


def feval_ld(x, Cm, W, ex=0.0):
    """(f, bound) of f = 1/2 sum am(x - Cm, W)^2 for an x known to within ex per entry"""
    N = x.size
    live = ~(np.abs(W) < W_USED)
    r = np.where(live, (np.asarray(x, dtype=LD) - Cm.astype(LD)) * W.astype(LD), LD(0))
    f = LD(0.5) * (r * r).sum()
    with np.errstate(invalid="ignore"):                                # an unbounded ex times a zero weight
        dr = np.where(live, np.abs(W) * ex, 0).astype(LD) + 2 * U * np.abs(r)
    bound = SLACK * ((np.abs(r) * dr).sum() + LD(0.5) * (dr * dr).sum() + (N + 2) * U * f)
    return f, bound


def gpmax_ld(x, Cm, W, thr):
    """(gpmax, bound) of max |proj(x - g) - x| with g = am(x - Cm, W), for a float64 x taken as exact"""
    x = np.asarray(x, dtype=np.float64)
    t = x - grad64(x, Cm, W)                                          # float64 as in the kernel: exact input of proj
    P, b = proj_ld(t, thr)
    gp = np.abs(P - x.astype(LD))
    return gp.max(), SLACK * (b.max() + U * gp.max())


def clamp_lmbda(gpmax, lmin, lmax):
    """the start's lambda, float64 as in the kernel"""
    return min(lmax, max(lmin, 1.0 / gpmax)) if gpmax > 1.0e-15 else 0.0


def bb_ld(x_old, x_new, Cm, W):
    """(sdots, sdoty, bound of sdoty, relative bound of sdots / sdoty) from two float64 iterates: s and y are float64 as in
    the kernel (bit-equal), only the two sums are the kernel's in another order.  Every product s_i y_i is >= 0 (W = m^2
    >= 0 and am is monotone in v), so sum |s_i y_i| = sdoty."""
    s = np.asarray(x_new, dtype=np.float64) - np.asarray(x_old, dtype=np.float64)
    y = grad64(x_new, Cm, W) - grad64(x_old, Cm, W)
    N = s.size
    ss, sy = s * s, s * y                                             # float64 products, as in the kernel
    sdots, sdoty = ss.astype(LD).sum(), sy.astype(LD).sum()
    b_sy = SLACK * N * U * np.abs(sy).astype(LD).sum()
    rel = SLACK * 2 * (N + 2) * U
    return sdots, sdoty, b_sy, rel


class Step(object):
    """what one iteration gives.  status: None (the iteration completed) or MAXFEV (the line search spent the budget; the
    state stays).  x, f, gpmax, lmbda: new state (longdouble), ex, ef, egp, elmbda: their bounds (ex per entry, elmbda
    absolute).  count: evaluations after the step.  decisions: list of (name, taken, margin, bound); a decision is safe
    when margin > bound.  paths: set of names of the branches gone through."""
    pass


def step_ld(x, g, lmbda, f, hist, count, it, Cm, W, P, elmbda=0.0):
    """One SPG iteration of the kernel from the float64 state (x, g = grad64(x), f, hist, count, it) with the step length
    lmbda known to within elmbda.  `it` is the iteration count BEFORE this step; hist is the ring as the kernel holds it
    (float64 values the kernel itself computed, -inf where unwritten); it is not modified: the new ring is in Step.hist."""
    x = np.asarray(x, dtype=np.float64)
    g = np.asarray(g, dtype=np.float64)
    M = x.shape[0]
    N = M * M
    thr, max_fevals, hlen = P["spd_threshold"], int(P["max_fevals"]), int(P["hlength"])
    lmin, lmax = float(P["lmbda_min"]), float(P["lmbda_max"])
    st = Step()
    dec, paths = [], set()
    it = it + 1
    xl, gl, lam = x.astype(LD), g.astype(LD), LD(lmbda)
    # d = proj(x - lmbda g) - x.  The kernel rounds x - lmbda g (2u per entry) with its own lmbda; proj does not expand
    # Frobenius distances, so the input's perturbation passes through at most at its Frobenius norm.
    tin = xl - lam * gl
    e_in = SLACK * (2 * U * np.sqrt(((np.abs(xl) + np.abs(lam * gl)) ** 2).sum()) + LD(elmbda) * np.sqrt((gl * gl).sum()))
    Pt, bP = proj_ld(tin, thr)
    d = Pt - xl
    ed = SLACK * (bP.max() + e_in + U * np.abs(d).max())              # per entry
    gd = (gl * d).sum()
    egd = SLACK * (np.abs(gl).sum() * ed + (N + 1) * U * np.abs(gl * d).sum())
    fmx = max(float(h) for h in hist[:hlen])                          # the kernel's own float64 values: exact
    fl = LD(f)
    alpha, ealpha = LD(1), LD(0)
    dmax = np.abs(d).max()

    def trial(alpha, ealpha):
        xn = xl + alpha * d
        exn = SLACK * (alpha * ed + ealpha * dmax + 2 * U * (np.abs(xl) + np.abs(alpha * d)).max())
        fn, efn = feval_ld(xn, Cm, W, exn)
        return xn, exn, fn, efn

    def armijo(fn, efn, alpha, ealpha):
        rhs = LD(fmx) + LD(GAMMA) * alpha * gd
        b = SLACK * (efn + GAMMA * (alpha * egd + ealpha * abs(gd)) + 3 * U * (abs(LD(fmx)) + GAMMA * abs(alpha * gd)))
        # what this test pins besides its own outcome: would it, beyond rounding, fall the other way with a sufficient-
        # decrease constant ten times as large, or with a window that had already dropped its oldest value (the slot this
        # iteration overwrites)?  A table whose tests all fall the same way either way cannot tell such a kernel apart.
        rhs10 = LD(fmx) + 10 * LD(GAMMA) * alpha * gd
        if (fn > rhs10) != (fn > rhs) and abs(fn - rhs10) > 10 * b:
            paths.add("ls:gamma_decides")
        if hlen > 1:
            rhs_w = max(float(h) for k, h in enumerate(hist[:hlen]) if k != it % hlen) + LD(GAMMA) * alpha * gd
            if (fn > rhs_w) != (fn > rhs) and abs(fn - rhs_w) > b:
                paths.add("ls:oldest_decides")
        return fn > rhs, abs(fn - rhs), b

    xn, exn, fn, efn = trial(alpha, ealpha)
    count += 1
    ntrial = 1
    while True:
        rejected, margin, b = armijo(fn, efn, alpha, ealpha)
        dec.append(("armijo", bool(rejected), margin, b))
        if not rejected:
            break
        dec.append(("count<max_fevals", count < max_fevals, LD(1), LD(0)))         # integers: exact
        if not count < max_fevals:
            break
        dec.append(("alpha<=sigma_min", bool(alpha <= SIGMA_MIN), abs(alpha - LD(SIGMA_MIN)), SLACK * (ealpha + U)))
        if alpha <= SIGMA_MIN:
            alpha, ealpha = alpha * LD(0.5), ealpha * LD(0.5)
            paths.add("ls:halve")
        else:
            num = LD(-0.5) * (alpha * alpha) * gd
            den = fn - fl - alpha * gd
            at = num / den
            eden = SLACK * (efn + alpha * egd + ealpha * abs(gd) + 3 * U * (abs(fn) + abs(fl) + abs(alpha * gd)))
            enum = SLACK * (abs(num) * (2 * ealpha / alpha + 4 * U) + LD(0.5) * alpha * alpha * egd)
            if eden < abs(den):
                eat = SLACK * (enum / abs(den) + abs(at) * eden / (abs(den) - eden) + U * abs(at))
            else:
                eat = LD("inf")                                       # the denominator's sign is not determined
            lo = at < SIGMA_MIN
            dec.append(("alpha_t<sigma_min", bool(lo), abs(at - LD(SIGMA_MIN)), eat))
            hi = at > LD(SIGMA_MAX) * alpha
            if not lo:
                dec.append(("alpha_t>sigma_max*alpha", bool(hi), abs(at - LD(SIGMA_MAX) * alpha), SLACK * (eat + ealpha + U)))
            if lo or hi:
                paths.add("ls:safeguard_lo" if lo else "ls:safeguard_hi")
                alpha, ealpha = LD(0.5) * alpha, LD(0.5) * ealpha
            else:
                paths.add("ls:quadratic")
                alpha, ealpha = at, eat
        xn, exn, fn, efn = trial(alpha, ealpha)
        count += 1
        ntrial += 1
    st.decisions, st.paths, st.count, st.it, st.ntrial = dec, paths, count, it, ntrial
    st.alpha, st.gd = alpha, gd
    if rejected:                                                      # the line search's own MAXFEV: the state stays
        paths.add("exit:maxfev_linesearch")
        st.status, st.x, st.ex, st.f, st.ef = MAXFEV, xl, LD(0), fl, LD(0)
        st.hist = list(hist)
        return st
    st.status = None
    if ntrial == 1:
        paths.add("ls:first_trial")
    if fn > fl:
        paths.add("ls:nonmonotone")
    st.x, st.ex, st.f, st.ef = xn, exn, fn, efn
    st.hist = list(hist)
    st.hist[it % hlen] = float(fn)
    # the rest is a function of the new point alone; the kernel evaluates it at ITS new point, which is within ex of xn
    x64 = xn.astype(np.float64)
    st.x64 = x64
    sdots, sdoty, b_sy, rel = bb_ld(x, x64, Cm, W)
    # moving the new point by ex per entry moves s by ex and y by |W| ex
    b_sy = SLACK * (b_sy + float(exn) * (np.abs(W) * np.abs(x64 - x) + np.abs(grad64(x64, Cm, W) - g)).sum())
    dec.append(("sdoty<=0", bool(sdoty <= 0), abs(sdoty), b_sy))
    st.sdots, st.sdoty = sdots, sdoty
    if sdoty <= 0:
        paths.add("lmbda:sdoty<=0")
        st.lmbda, st.elmbda = LD(lmax), LD(0)
    else:
        r = sdots / sdoty
        if r > lmax: paths.add("lmbda:clamped_max")
        elif r < lmin: paths.add("lmbda:clamped_min")
        else: paths.add("lmbda:bb")
        st.lmbda = min(LD(lmax), max(LD(lmin), r))
        st.elmbda = LD(0) if (r > lmax or r < lmin) else r * rel
    st.gpmax, st.egp = gpmax_ld(x64, Cm, W, thr)
    st.egp = SLACK * (st.egp + 2 * float(exn) * np.sqrt(LD(N)))       # x and x - g move with the new point; proj is nonexpansive
    return st


class Run(object):
    """rc; per call X (float64), f, gpmax (longdouble), it, count, info; steps: the Step of every iteration; decisions: every
    (where, name, taken, margin, bound); paths: the union of the branches gone through"""
    pass


def check_args(M, n_out, P):
    ok = (1 <= M <= MAX_MODELS and 1 <= n_out <= MAX_OUTPUTS and 1 <= int(P["hlength"]) <= MAX_HISTORY
          and np.isfinite(P["spd_threshold"]) and np.isfinite(P["eps"]) and not np.isnan(P["lmbda_min"])
          and not np.isnan(P["lmbda_max"]) and int(P["maxit"]) >= 0 and int(P["max_fevals"]) >= 0)
    return RC_OK if ok else ERR_ARG


def run_ld(C, mask, params=None, max_steps=None):
    """bluest_cov_project for ONE output.  max_steps: stop the restatement after so many iterations (the run is then not
    finished: info is None) -- for the rows of which only the first iterations are compared."""
    P = dict(default_params)
    P.update(params or {})
    C = np.asarray(C, dtype=np.float64)
    M = C.shape[0]
    R = Run()
    R.steps, R.decisions, R.paths = [], [], set()
    R.rc = check_args(M, 1, P)
    if R.rc:
        return R
    Cm, W, unknown, bad = prepare(C, mask)
    thr, eps, maxit, max_fevals = P["spd_threshold"], float(P["eps"]), int(P["maxit"]), int(P["max_fevals"])
    if bad:
        R.X, R.f, R.gpmax, R.it, R.count, R.info = C.copy(), LD("nan"), LD("nan"), 0, 0, NONFINITE
        R.paths.add("status:nonfinite")
        return R
    if (~(np.abs(np.asarray(mask, dtype=np.float64)) < MASK_USED) & (np.abs(W) < W_USED)).any():
        R.paths.add("mask:thresholds_differ")
    if not unknown:
        X, b = proj_ld(C, thr, lower_only=True)
        R.X, R.eX = X, b
        R.f = np.sqrt(((C.astype(LD) - X) ** 2).sum())
        R.gpmax, R.it, R.count, R.info = LD(0), 0, 0, OK
        R.paths.update(["clip", "status:ok"])
        if not np.array_equal(C, C.T):
            R.paths.add("clip:lower_only")
        return R
    R.paths.add("spg:odd_M" if M & 1 else "spg:even_M")
    x0, b0 = proj_ld(Cm, thr)
    x0 = x0.astype(np.float64)                                        # the kernel's x is float64 in memory
    x1, b1 = proj_ld(x0, thr)
    R.ex0 = SLACK * (b1 + np.sqrt((b0 * b0).sum()) + U * np.abs(x1))  # proj does not expand the first projection's error
    x = x1.astype(np.float64)
    f, _ = feval_ld(x, Cm, W)
    f = float(f)
    g = grad64(x, Cm, W)
    it, count = 0, 1
    hist = [f] + [-np.inf] * (int(P["hlength"]) - 1)
    gpmax, egp = gpmax_ld(x, Cm, W, thr)
    R.x0, R.f0, R.gpmax0, R.egp0 = x.copy(), f, gpmax, egp
    R.decisions.append((0, "gpmax>1e-15", bool(gpmax > 1e-15), abs(gpmax - LD(1e-15)), egp))
    lmbda = LD(clamp_lmbda(float(gpmax), float(P["lmbda_min"]), float(P["lmbda_max"])))
    if gpmax > 1e-15:
        r = 1.0 / float(gpmax)
        R.paths.add("lmbda:clamped_max" if r > P["lmbda_max"] else "lmbda:clamped_min" if r < P["lmbda_min"] else "lmbda:start")
    R.lmbdas = [lmbda]
    finished = True
    while True:
        R.decisions.append((it, "gpmax>eps", bool(gpmax > eps), abs(gpmax - LD(eps)), egp))
        if not gpmax > eps: break
        if not it < maxit: break
        R.decisions.append((it, "count<max_fevals", count < max_fevals, LD(1), LD(0)))
        if not count < max_fevals: break
        if max_steps is not None and it >= max_steps:
            finished = False
            break
        st = step_ld(x, g, lmbda, f, hist, count, it, Cm, W, P)
        R.steps.append(st)
        R.paths |= st.paths
        it, count = st.it, st.count
        R.decisions += [(it,) + d for d in st.decisions]
        if st.status == MAXFEV:
            R.X, R.f, R.gpmax, R.it, R.count, R.info = x, LD(f), gpmax, it, count, MAXFEV
            R.paths.add("status:maxfev")
            return R
        x, f, hist = st.x64, float(st.f), st.hist
        g = grad64(x, Cm, W)
        gpmax, egp, lmbda = st.gpmax, st.egp, st.lmbda
        R.lmbdas.append(lmbda)
    R.X, R.f, R.gpmax, R.it, R.count = x, LD(f), gpmax, it, count
    if not finished:
        R.info = None
    elif gpmax <= eps:
        R.info = OK
    elif it >= maxit:
        R.info = MAXIT
    else:
        R.info = MAXFEV
        R.paths.add("exit:maxfev_loop")
    if R.info is not None:
        R.paths.add("status:" + {OK: "ok", MAXIT: "maxit", MAXFEV: "maxfev"}[R.info])
    return R


def margins_hold(decisions):
    """the decisions whose margin does not exceed its bound"""
    return [d for d in decisions if not d[-2] > d[-1]]

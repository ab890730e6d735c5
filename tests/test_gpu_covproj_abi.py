"""
GPU tests of bluest_cov_project (csrc/covproj.hip) at its own interface, called through ctypes, against the longdouble
restatement oracle/covproj_ref.py on the case table tests/covproj_cases.py (whose soundness and coverage
test_covproj_ref.py checks on the CPU).  Everything a call writes is compared: X, f, gpmax, it, count, info.

The SPG rows are compared in lock-step: the kernel is deterministic, so a call with maxit = k returns its state after k
iterations.  From the calls k = 0..K the test recovers x_k, f_k (hence the history ring), count_k, g_k (a float64 function
of x_k) and the step length the kernel used (from x_k, x_{k-1}), gives that state to step_ld and compares the result with
the kernel's own state after k + 1 iterations: no error accumulates, and a wrong branch shows at the step where it is taken.

Every bound is the reference's (derived in oracle/covproj_ref.py); the largest ratio of error to bound is printed per test.
"""
import ctypes

import numpy as np
import pytest

import covproj_cases as cc
from oracle import covproj_ref as ref

pytestmark = pytest.mark.gpu
LD = np.longdouble
RATIOS = {}


@pytest.fixture(autouse=True, scope="module")
def _library():
    from bluest_amd import build
    build.build()
    yield
    for k in sorted(RATIOS):
        print("largest error / bound, %s: %.3g" % (k, RATIOS[k]))


def ratio(kind, err, bound):
    with np.errstate(invalid="ignore", divide="ignore"):
        r = np.where(np.asarray(err, dtype=LD) == 0, LD(0), np.asarray(err, dtype=LD) / np.asarray(bound, dtype=LD))
    r = float(np.max(r))
    RATIOS[kind] = max(RATIOS.get(kind, 0.0), r)
    return r


def call(Cs, masks, params=None, null=None, M=None, n_out=None):
    """(rc, [(X, f, gpmax, it, count, info) per output]) of one call; outputs are poisoned first"""
    from bluest_amd import _lib
    P = dict(ref.default_params)
    P.update(params or {})
    Cs = np.ascontiguousarray(np.array(Cs, dtype=np.float64))
    masks = np.ascontiguousarray(np.array(masks, dtype=np.float64))
    n, m = Cs.shape[0], Cs.shape[1]
    X = np.full_like(Cs, -7.0)
    f, gp = np.full(n, -7.0), np.full(n, -7.0)
    it, count, info = np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int64), np.full(n, -7, dtype=np.int32)
    ptrs = {"C": Cs, "mask": masks, "X": X, "f": f, "gpmax": gp, "it": it, "count": count, "info": info}
    a = {k: (None if k == null else _lib.ptr(v)) for k, v in ptrs.items()}
    rc = _lib.lib().bluest_cov_project(m if M is None else M, n if n_out is None else n_out, a["C"], a["mask"],
                                       ctypes.c_double(P["spd_threshold"]), ctypes.c_double(P["eps"]),
                                       ctypes.c_double(P["lmbda_min"]), ctypes.c_double(P["lmbda_max"]), int(P["maxit"]),
                                       int(P["max_fevals"]), int(P["hlength"]), a["X"], a["f"], a["gpmax"], a["it"], a["count"],
                                       a["info"], None)
    return rc, [(X[o], float(f[o]), float(gp[o]), int(it[o]), int(count[o]), int(info[o])) for o in range(n)]


def solo(row, **change):
    rc, out = call([row["C"]], [row["mask"]], dict(row["params"], **change))
    assert rc == ref.RC_OK
    return out[0]


def _ids(group):
    return [r["name"] for r in cc.by_group(group)]


# ---- the single clip -------------------------------------------------------------------------------------------------------
def check_clip(row, R):
    X, f, gpmax, it, count, info = solo(row)
    assert (gpmax, it, count, info) == (0.0, 0, 0, ref.OK)
    assert np.array_equal(X, X.T)
    r = ratio("clip X", np.abs(X - R.X), R.eX)
    print("%s: X error / bound %.3g" % (row["name"], r))
    assert r <= 1.0
    # f = ||C - X||_F against the full C: X moves within its bound, the sum of N squares and the root round
    C = row["C"]
    N = C.size
    fb = np.sqrt((R.eX ** 2).sum()) + (N + 4) * ref.U * R.f
    if np.isfinite(float(((C - X) ** 2).sum())) and float(R.f) > 1e-150:
        assert ratio("clip f", abs(LD(f) - R.f), fb) <= 1.0, (f, R.f)
    return X


@pytest.mark.parametrize("name", _ids("clip"))
def test_single_clip(name):
    row = cc.case(name)
    R = cc.reference(name)
    X = check_clip(row, R)
    if "_spd_" in name:                                               # nothing clipped: X = C within the bound
        assert (np.abs(X - row["C"]) <= R.eX).all()
    if "asymmetric" in name:                                          # the strict upper triangle is never read
        C2 = np.tril(row["C"]) + np.tril(row["C"], -1).T
        X2 = solo(dict(row, C=C2))[0]
        assert np.array_equal(X, X2)


def test_overflowing_norm_is_scaled():
    """M = 4, entries near 1e155: sum a^2 is inf in float64.  Before proj() scaled its norm the tolerance was inf, no rotation
    was taken and the kernel returned diag(clip(diag C)) with status OK."""
    row = cc.overflow_case()
    R = cc.reference(row["name"])
    X, f, gpmax, it, count, info = solo(row)
    if info == ref.OK:
        r = ratio("clip X", np.abs(X - R.X), R.eX)
        print("overflow: X error / bound %.3g, f %r" % (r, f))
        assert r <= 1.0
        assert (gpmax, it, count) == (0.0, 0, 0)
    else:
        assert info in (ref.NONFINITE, ref.NOEIG)


# ---- SPG, lock-step ----------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", _ids("spg"))
def test_spg_lock_step(name):
    row = cc.case(name)
    R = cc.reference(name)                                            # the reference's own run: the branches to expect
    Cm, W, unknown, bad = ref.prepare(row["C"], row["mask"])
    P = dict(ref.default_params, **row["params"])
    K = row["K"]
    states = [solo(row, maxit=k) for k in range(K + 1)]
    # k = 0: x0 = proj(proj(mask o C)), f, gpmax of the start
    X0, f0, gp0, it0, count0, info0 = states[0]
    assert (it0, count0) == (0, 1)
    assert ratio("spg x0", np.abs(X0 - R.x0), R.ex0) <= 1.0
    fr, fb = ref.feval_ld(X0, Cm, W)
    assert ratio("spg f(x)", abs(LD(f0) - fr), fb + ref.U * fr) <= 1.0
    gr, gb = ref.gpmax_ld(X0, Cm, W, P["spd_threshold"])
    assert ratio("spg gpmax(x)", abs(LD(gp0) - gr), gb) <= 1.0
    hist = [f0] + [-np.inf] * (P["hlength"] - 1)
    lmbda, elmbda = ref.clamp_lmbda(gp0, P["lmbda_min"], P["lmbda_max"]), 0.0      # float64 as the kernel: exact
    steps = 0
    for k in range(K):
        Xk, fk, gpk, itk, countk, infok = states[k]
        Xn, fn, gpn, itn, countn, infon = states[k + 1]
        if not gpk > P["eps"]:                                        # converged: every later call returns this state
            assert infok == ref.OK and np.array_equal(Xn, Xk) and (fn, gpn, itn, countn, infon) == (fk, gpk, itk, countk, infok)
            continue
        assert itk == k and infok == ref.MAXIT
        st = ref.step_ld(Xk, ref.grad64(Xk, Cm, W), lmbda, fk, hist, countk, itk, Cm, W, P, elmbda=elmbda)
        unsafe = ref.margins_hold(st.decisions)
        assert not unsafe, (k, [(d[0], float(d[-2]), float(d[-1])) for d in unsafe])
        assert st.status is None
        assert itn == k + 1 and countn - countk == st.count - countk, (k, countn - countk, st.count - countk)
        assert st.paths == R.steps[k].paths, (k, st.paths, R.steps[k].paths)
        rx = ratio("spg x step", np.abs(Xn - st.x), st.ex)
        rf = ratio("spg f step", abs(LD(fn) - st.f), st.ef)
        rg = ratio("spg gpmax step", abs(LD(gpn) - st.gpmax), st.egp)
        assert max(rx, rf, rg) <= 1.0, (k, rx, rf, rg)
        # f and gpmax as functions of the kernel's own new point: no step error in these two
        fr, fb = ref.feval_ld(Xn, Cm, W)
        assert ratio("spg f(x)", abs(LD(fn) - fr), fb + ref.U * fr) <= 1.0, k
        gr, gb = ref.gpmax_ld(Xn, Cm, W, P["spd_threshold"])
        assert ratio("spg gpmax(x)", abs(LD(gpn) - gr), gb) <= 1.0, k
        # the state for the next step, from the kernel's own values
        hist = list(hist)
        hist[(k + 1) % P["hlength"]] = fn
        sdots, sdoty, b_sy, rel = ref.bb_ld(Xk, Xn, Cm, W)
        assert sdoty > b_sy
        r = sdots / sdoty
        lmbda = min(LD(P["lmbda_max"]), max(LD(P["lmbda_min"]), r))
        elmbda = 0.0 if (r > P["lmbda_max"] or r < P["lmbda_min"]) else r * rel
        steps += 1
    assert steps == len(R.steps)
    X, f, gp, it, count, info = states[K]
    if R.info == ref.OK:                                              # converged inside K
        assert (it, count, info) == (R.it, R.count, ref.OK)
    else:
        assert (it, count, info) == (K, R.count, ref.MAXIT)
    print("%s: %d steps compared, it %d count %d" % (name, steps, it, count))


# ---- budgets and states ----------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("name", [b[0]["name"] for b in cc.budget_cases()])
def test_budgets_and_states(name):
    row, info_e, it_e, count_e, _ = next(b for b in cc.budget_cases() if b[0]["name"] == name)
    R = cc.reference(name)
    X, f, gpmax, it, count, info = solo(row)
    assert (info, it, count) == (R.info, R.it, R.count) and info == info_e
    if info == ref.NONFINITE:
        assert np.array_equal(X, row["C"], equal_nan=True) and np.isnan(f) and np.isnan(gpmax)
        return
    # X, f, gpmax are the state after the last completed iteration: the same bits as the call that stops there by maxit.
    # The line search's own exit counts the iteration it gave up in, and x stays the last accepted point.
    done = it - 1 if name == "maxfev2_overshoot" else it
    Xk, fk, gpk, itk, countk, _ = solo(row, maxit=done, max_fevals=ref.default_params["max_fevals"])
    assert itk == done and np.array_equal(X, Xk) and (f, gpmax) == (fk, gpk)
    Cm, W, _, _ = ref.prepare(row["C"], row["mask"])
    fr, fb = ref.feval_ld(X, Cm, W)
    assert ratio("spg f(x)", abs(LD(f) - fr), fb + ref.U * fr) <= 1.0
    if it == 0:
        assert ratio("spg x0", np.abs(X - R.x0), R.ex0) <= 1.0


# ---- one launch, many outputs ------------------------------------------------------------------------------------------------
def same(a, b):
    return (np.array_equal(a[0], b[0], equal_nan=True) and np.array([a[1], a[2]]).tobytes() == np.array([b[1], b[2]]).tobytes()
            and a[3:] == b[3:])


def test_five_outputs_in_five_states():
    cases = cc.multi_case()
    rc, outs = call([c[1] for c in cases], [c[2] for c in cases], cc.MULTI_PARAMS)
    assert rc == ref.RC_OK
    assert [o[5] for o in outs] == [c[3] for c in cases]
    assert outs[0][3:5] == (0, 0) and outs[1][3] > 0
    for (name, C, mask, info), o in zip(cases, outs):
        rc, (s,) = call([C], [mask], cc.MULTI_PARAMS)
        assert rc == ref.RC_OK and same(o, s), name


def test_1024_outputs():
    Cs, masks = [], []
    for o in range(1024):
        Cs.append(cc.indefinite(3, 3000 + o, nneg=1))
        masks.append(np.ones((3, 3)) if o % 4 == 0 else cc.mask01(3, o, 0.4))
    P = {"maxit": 20, "max_fevals": 60}
    rc, outs = call(Cs, masks, P)
    assert rc == ref.RC_OK
    assert {o[5] for o in outs} >= {ref.OK, ref.MAXIT}
    for o in range(1024):
        rc, (s,) = call([Cs[o]], [masks[o]], P)
        assert rc == ref.RC_OK and same(outs[o], s), o


# ---- argument errors -------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing():
    C, m = [np.eye(3)], [np.ones((3, 3))]
    bad = [dict(M=0), dict(M=65), dict(n_out=0), dict(n_out=1025), dict(params={"hlength": 0}), dict(params={"hlength": 65}),
           dict(params={"eps": float("nan")}), dict(params={"maxit": -1})]
    bad += [dict(null=k) for k in ("C", "mask", "X", "f", "gpmax", "it", "count", "info")]
    for kw in bad:
        rc, (o,) = call(C, m, **kw)
        assert rc == ref.ERR_ARG, kw
        assert (o[0] == -7.0).all() and o[1:] == (-7.0, -7.0, -7, -7, -7), kw       # nothing written
    rc, (o,) = call(C, m)
    assert rc == ref.RC_OK and o[5] == ref.OK

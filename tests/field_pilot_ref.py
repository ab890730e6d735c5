"""numpy restatement of include/bluest_hip.h, Part 17 (bluest_field_pilot_moments): every operation in the order the header
states, so the results have the kernel's bits; the long-double two-pass values; the forward error bounds the tests use; and the
stand-in the host tests put in place of the GPU call.

THE BOUNDS (u = 2^-53, first order, doubled to cover the second-order terms).  With a, b, t the exact centred values:
  q_s:  a, b and w_c a carry one rounding each and the fma chain over the <= d components of a sample (strips joined) adds at most
        d more per term, so |q^_s - q_s| <= E_s = (d + 4) u A_s with A_s = sum_c w_c |a| |b|; for r_s the same with |t| |t|.
  u_s = q_s - q_0 is formed with one rounding:       |u^_s - u_s| <= e_s = E_s + E_0 + u |u_s|.
  S1 = sum u_s, N additions in chunks:               |S1^ - S1| <= dS1 = sum e_s + (N + 1) u sum |u_s|.
  S2 = sum u_s^2, an fma chain in chunks:            |S2^ - S2| <= dS2 = sum 2 |u_s| e_s + (N + 2) u sum u_s^2.
  V = S2 - S1^2 / N:                                 |V^ - V| <= dV = dS2 + 2 |S1| dS1 / N + 3 u (S2 + S1^2 / N).
  SE = sqrt(max(V, 0) / (N (N - 1))):                |SE^ - SE| <= min(dV / sqrt(V), sqrt(dV)) / sqrt(N (N - 1)) + 3 u SE
        (|sqrt(x) - sqrt(y)| <= |x - y| / sqrt(y) and <= sqrt(|x - y|)).
"""
import math

import numpy as np

import gsums_ref
from gsums_ref import same_bits  # noqa: F401
from pilot_ref import LD, U

CHUNK = 128                 # BLUEST_PILOT_CHUNK
STRIP = 512                 # BLUEST_FIELD_STRIP

def _libm_fma():
    """the C library's fma (correctly rounded, IEEE for NaN / Inf): some twenty times faster than exact rational arithmetic"""
    import ctypes
    import ctypes.util
    try:
        f = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6").fma
    except (OSError, AttributeError):
        return None
    f.restype, f.argtypes = ctypes.c_double, [ctypes.c_double] * 3
    return f if f(1.0 + 2.0 ** -52, 1.0 - 2.0 ** -52, -1.0) == -2.0 ** -104 else None


_exact = getattr(math, "fma", None) or _libm_fma()


def _fma1(a, b, c):
    """round(a * b + c) with one rounding; NaN / Inf operands give what IEEE arithmetic gives (a NaN, or the infinity)"""
    if _exact is not None:
        return _exact(a, b, c)
    if math.isfinite(a) and math.isfinite(b) and math.isfinite(c):
        return gsums_ref.fma(a, b, c)
    return a * b + c


_fma = np.frompyfunc(_fma1, 3, 1)


def fma(a, b, c):
    return _fma(a, b, c).astype(np.float64)


def _host(values):
    return np.asarray(values.cpu().numpy() if hasattr(values, "data_ptr") else values, dtype=np.float64)


def per_sample(values, w, centre, differences=True):
    """(q [N, P], r [N, P] or None, lo, hi) over the pairs lo <= hi with the kernel's bits: per strip the fma chain over ascending
    components from +0.0, the strips added in ascending order from +0.0"""
    Y, w, ce = _host(values), np.asarray(w, dtype=np.float64), np.asarray(centre, dtype=np.float64)
    N, L, d = Y.shape
    lo, hi = np.triu_indices(L)
    q, r = np.zeros((N, len(lo))), (np.zeros((N, len(lo))) if differences else None)
    with np.errstate(invalid="ignore", over="ignore"):
        for c0 in range(0, d, STRIP):
            p, pr = np.zeros((N, len(lo))), np.zeros((N, len(lo)))
            for c in range(c0, min(c0 + STRIP, d)):
                yi, yj, ci, cj = Y[:, lo, c], Y[:, hi, c], ce[lo, c], ce[hi, c]
                a, b = yi - ci, yj - cj
                p = fma(w[c] * a, b, p)
                if differences:
                    t = (yi - yj) - (ci - cj)
                    pr = fma(w[c] * t, t, pr)
            q = q + p
            if differences:
                r = r + pr
    return q, r, lo, hi


def _shifted_sums(q):
    """(q_0, S1, S2) [P] of q [N, P]: per chunk u = q_s - q_0, s1 = s1 + u, s2 = fma(u, u, s2) from +0.0; chunks added from +0.0"""
    N = q.shape[0]
    S1, S2 = np.zeros(q.shape[1]), np.zeros(q.shape[1])
    with np.errstate(invalid="ignore", over="ignore"):
        for s0 in range(0, N, CHUNK):
            s1, s2 = np.zeros(q.shape[1]), np.zeros(q.shape[1])
            for s in range(s0, min(s0 + CHUNK, N)):
                u = q[s] - q[0]
                s1 = s1 + u
                s2 = fma(u, u, s2)
            S1, S2 = S1 + s1, S2 + s2
    return q[0].copy(), S1, S2


def pilot_moments(values, w, centre, differences=True):
    """(qfirst, qs1, qs2, rfirst, rs1, rs2) [L, L] with the bits of bluest_field_pilot_moments: q symmetric, r at i < j else 0"""
    q, r, lo, hi = per_sample(values, w, centre, differences)
    L = int(np.shape(values)[1])
    out = []
    for a in _shifted_sums(q):
        m = np.zeros((L, L))
        m[lo, hi] = a
        m[hi, lo] = a
        out.append(m)
    if not differences:
        return tuple(out) + (None, None, None)
    off = lo < hi
    for a in _shifted_sums(r):
        m = np.zeros((L, L))
        m[lo[off], hi[off]] = a[off]
        out.append(m)
    return tuple(out)


def field_pilot_moments(values, w, centre=None, differences=True, slab_bytes=None, scratch_bytes=None):
    """stand-in for bluest_amd.field_pilot_errors.field_pilot_moments with the same bits (the default centre: the long-double
    mean rounded to float64, as the stand-in fields_ref.field_statistics gives it)"""
    Y = _host(values)
    if centre is None:
        centre = np.asarray(Y.astype(LD).sum(axis=0), dtype=np.float64) / Y.shape[0]
    return pilot_moments(Y, w, centre, differences)


# ---- long double ---------------------------------------------------------------------------------------------------------------
def per_sample_ld(values, w, centre):
    """(q [N, L, L], r [N, L, L], A [N, L, L], B [N, L, L]) in long double: the per-sample inner products of the centred values
    and of the centred explicit differences, and the same sums of the absolute terms"""
    Y, w, ce = _host(values).astype(LD), np.asarray(w, dtype=np.float64).astype(LD), np.asarray(centre, dtype=np.float64).astype(LD)
    X = Y - ce
    T = (Y[:, :, None, :] - Y[:, None, :, :]) - (ce[:, None, :] - ce[None, :, :])
    q, A = np.einsum("sic,c,sjc->sij", X, w, X), np.einsum("sic,c,sjc->sij", np.abs(X), w, np.abs(X))
    r = np.einsum("sijc,c,sijc->sij", T, w, T)
    return q, r, A, r.copy()


def two_pass_ld(x):
    """(mean, sum of squared deviations from it) over axis 0, in long double"""
    mean = x.sum(axis=0) / x.shape[0]
    return mean, ((x - mean) ** 2).sum(axis=0)


def standard_errors_ld(values, w, centre):
    """(SE(C^) [L, L], SE(dV^) [L, L]) in long double by the two-pass formula (N >= 2)"""
    q, r, _, _ = per_sample_ld(values, w, centre)
    N = q.shape[0]
    return tuple(np.sqrt(two_pass_ld(x)[1] / (LD(N) * (N - 1))) for x in (q, r))


def shifted_ld(x):
    """(x_0, sum (x_s - x_0), sum (x_s - x_0)^2) in long double"""
    u = x - x[0]
    return x[0], u.sum(axis=0), (u * u).sum(axis=0)


def bounds(values, w, centre):
    """per entry [L, L] and for q and r: (dfirst, dS1, dS2, dSE) as derived above, float64"""
    q, r, A, B = per_sample_ld(values, w, centre)
    N, d = q.shape[0], np.shape(values)[2]
    out = []
    for x, mag in ((q, A), (r, B)):
        E = 2 * (d + 4) * U * mag
        u = np.abs(x - x[0])
        e = E + E[0] + 2 * U * u
        S1, S2 = np.abs((x - x[0]).sum(axis=0)), (u * u).sum(axis=0)
        dS1 = e.sum(axis=0) + 2 * (N + 1) * U * u.sum(axis=0)
        dS2 = (2 * u * e).sum(axis=0) + 2 * (N + 2) * U * S2
        dV = dS2 + 2 * S1 * dS1 / N + 6 * U * (S2 + S1 * S1 / N)
        V = np.maximum(S2 - S1 * S1 / N, 0)
        if N >= 2:
            with np.errstate(divide="ignore", invalid="ignore"):
                dSE = np.minimum(np.where(V > 0, dV / np.sqrt(V), np.inf), np.sqrt(dV)) / np.sqrt(LD(N) * (N - 1))
            dSE = dSE + 3 * U * np.sqrt(V / (LD(N) * (N - 1)))
        else:
            dSE = np.full(V.shape, np.nan)
        out.append(tuple(np.asarray(a, dtype=np.float64) for a in (E[0], dS1, dS2, dSE)))
    return out

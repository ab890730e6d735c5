"""numpy restatement of Part 14 of include/bluest_hip.h (bluest_pilot_moments4) and of the standard errors made of it.

The eight sums are restated in long double FROM THE FLOAT64 TERMS' INPUTS: d = y - a and t = (y_i - y_j) - (a_i - a_j) are formed in
float64 exactly as the header states them (one rounding for d, three for t), and everything after that -- the products and the
sums -- is long double.  t has to be taken rounded: each of its inner differences is rounded relative to ITS OWN size, which for
two models with different means is far larger than |t|, so no bound in terms of sum|t^k| could hold against an exact t; that
rounding is part of the definition of the output, as it is in Part 10.  The bounds are stated in the sums of the absolute terms.

The standard errors are restated independently of the shifted one-pass form: two passes in long double about the sample mean.
"""
import numpy as np

LD = np.longdouble
U = 2.0 ** -53


def terms(values, shift=None):
    """(d [n, N, L], t [n, N, L, L]) in float64 as the kernel forms them; shift None = the first sample"""
    Y = np.ascontiguousarray(values, dtype=np.float64)
    a = Y[:, 0, :] if shift is None else np.asarray(shift, dtype=np.float64)
    d = Y - a[:, None, :]
    t = (Y[:, :, :, None] - Y[:, :, None, :]) - (a[:, :, None] - a[:, None, :])[:, None, :, :]
    return d, t


def _sums(d, t, differences):
    """first, s11, s21, s22, tpow of long-double terms"""
    d2 = d * d
    first = d.sum(axis=1)
    s11 = np.einsum("nsi,nsj->nij", d, d)
    s21 = np.einsum("nsi,nsj->nij", d2, d)
    s22 = np.einsum("nsi,nsj->nij", d2, d2)
    tpow = None
    if differences:
        upper = np.triu(np.ones(t.shape[2:]), 1).astype(LD)
        t2 = t * t
        tpow = np.stack([t.sum(axis=1), t2.sum(axis=1), (t2 * t).sum(axis=1), (t2 * t2).sum(axis=1)], axis=1) * upper
    return first, s11, s21, s22, tpow


def sums_ld(values, shift=None, differences=True):
    """(first [n, L], s11, s21, s22 [n, L, L], tpow [n, 4, L, L]) in long double"""
    d, t = terms(values, shift)
    return _sums(d.astype(LD), t.astype(LD), differences)


def abs_sums_ld(values, shift=None, differences=True):
    """the sums of the absolute values of the same terms"""
    d, t = terms(values, shift)
    return _sums(np.abs(d).astype(LD), np.abs(t).astype(LD), differences)


def bounds(values, shift=None, differences=True):
    """(N + 16) u sum|term| per sum: at most N - 1 additions inside the chunks and one per chunk, at most 8 roundings inside a
    term (d once each, p or q, the product); 16 leaves slack"""
    N = np.shape(values)[1]
    return tuple(None if a is None else np.asarray((N + 16) * U * a, dtype=np.float64) for a in abs_sums_ld(values, shift, differences))


def pilot_fourth_moments(values, differences=True, shift=None, slab_bytes=None):
    """stand-in for bluest_amd.pilot_errors.pilot_fourth_moments: the long-double sums rounded to float64"""
    values = np.asarray(values, dtype=np.float64)
    used = values[:, 0, :].copy() if shift is None else np.asarray(shift, dtype=np.float64)
    return (used,) + tuple(None if s is None else np.asarray(s, dtype=np.float64) for s in sums_ld(values, shift, differences))


def standard_errors(values):
    """(SE(C^) [n, L, L], SE(dV^) [n, L, L], NaN outside i < j) of the 1/N estimates, two passes in long double:
    Var(s_ij) = mu22 / N - (N - 2) mu11^2 / (N (N - 1)) + mu20 mu02 / (N (N - 1)) and Var(s^2) = mu4 / N - (N - 3) mu2^2 / (N (N - 1))
    for the unbiased estimates, times ((N - 1) / N)^2 for the 1/N ones"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    n, N, L = Y.shape
    if N < 2:
        return np.full((n, L, L), np.nan), np.full((n, L, L), np.nan)
    Z = Y - Y.mean(axis=1, keepdims=True)
    mu11 = np.einsum("nsi,nsj->nij", Z, Z) / N
    mu22 = np.einsum("nsi,nsj->nij", Z * Z, Z * Z) / N
    var = np.diagonal(mu11, axis1=1, axis2=2)
    v = mu22 / N - (N - 2) * mu11 ** 2 / (N * (N - 1)) + var[:, :, None] * var[:, None, :] / (N * (N - 1))
    se_c = (N - 1) / LD(N) * np.sqrt(np.maximum(v, 0))
    D = Y[:, :, :, None] - Y[:, :, None, :]
    D = D - D.mean(axis=1, keepdims=True)
    mu2, mu4 = (D ** 2).mean(axis=1), (D ** 4).mean(axis=1)
    v = mu4 / N - (N - 3) * mu2 ** 2 / (N * (N - 1))
    se_d = np.asarray((N - 1) / LD(N) * np.sqrt(np.maximum(v, 0)), dtype=np.float64)
    se_d[:, ~np.triu(np.ones((L, L), dtype=bool), 1)] = np.nan
    return np.asarray(se_c, dtype=np.float64), se_d


def estimates(values):
    """(C^ [n, L, L], dV^ [n, L, L]) with the 1/N normalisation, two passes in long double"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    Z = Y - Y.mean(axis=1, keepdims=True)
    D = Y[:, :, :, None] - Y[:, :, None, :]
    D = D - D.mean(axis=1, keepdims=True)
    return (np.asarray(np.einsum("nsi,nsj->nij", Z, Z) / Y.shape[1], dtype=np.float64),
            np.asarray((D ** 2).mean(axis=1), dtype=np.float64))


def chunked_f64(values, shift=None, chunk=128):
    """float64 emulation of the chunked order WITHOUT fma (numpy has none): not the kernel's bits, but the same order of additions;
    (first, s11, s21, s22, tpow)"""
    d, t = terms(values, shift)
    a, b = d[:, :, :, None], d[:, :, None, :]
    p = a * b
    upper = np.triu(np.ones(t.shape[2:]), 1)
    q = t * t
    series = [d, p, a * p, p * p, t * upper, q * upper, q * t * upper, q * q * upper]
    out = []
    for T in series:
        total = np.zeros(T.shape[:1] + T.shape[2:])
        for c in range(0, T.shape[1], chunk):
            acc = np.zeros_like(total)
            for s in range(c, min(c + chunk, T.shape[1])):
                acc = acc + T[:, s]
            total = total + acc
        out.append(total)
    return out[0], out[1], out[2], out[3], np.stack(out[4:], axis=1)

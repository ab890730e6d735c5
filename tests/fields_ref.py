"""numpy restatement of the two summation orders of include/bluest_hip.h, Part 12 (bluest_field_stats, bluest_field_sums): every
addition in the order the header states, so the results have the kernels' bits; the long-double sums with the sums of the
absolute terms the rounding bounds are stated in; and the stand-ins the host tests put in place of the GPU calls."""
import numpy as np

import gsums_ref
from gsums_ref import same_bits  # noqa: F401
from pilot_ref import LD, U

CHUNK = 128                 # BLUEST_PILOT_CHUNK
TILE = 8                    # BLUEST_FIELD_TILE
LANES = 64

_fma = np.frompyfunc(gsums_ref.fma, 3, 1)


def fma(a, b, c):
    """elementwise round(a * b + c) with one rounding (finite operands)"""
    return _fma(a, b, c).astype(np.float64)


def tree(lanes):
    """for off = 32 .. 1, lane l < off takes p[l] + p[l + off]; the result is lane 0's"""
    p = list(lanes)
    off = LANES // 2
    while off > 0:
        for l in range(off):
            p[l] = p[l] + p[l + off]
        off //= 2
    return p[0]


def pairs(L):
    """the pairs i < j in row-major order, the rows of the ABI's sumsd1"""
    return np.triu_indices(L, 1)


def field_stats(values, w, differences=True):
    """(sumse [L, d], sumsc [L, L], sumsd1 [P, d], sumsd2 [L, L]) of values [N, L, d] with the bits of bluest_field_stats"""
    Y = np.asarray(values, dtype=np.float64)
    w = np.asarray(w, dtype=np.float64)
    N, L, d = Y.shape
    iu = np.triu_indices(L)                                             # i <= j: what the kernel accumulates, mirrored at the end
    lo, hi = iu
    su = pairs(L)
    sumse, flat = np.zeros((L, d)), np.zeros((len(su[0]), d))
    pc, qc = np.zeros(len(lo)), np.zeros(len(lo))
    for s0 in range(0, N, CHUNK):
        block = Y[s0:s0 + CHUNK]
        e, r = np.zeros((L, d)), np.zeros((len(su[0]), d))
        for y in block:                                                 # per (model or pair, component): ascending samples
            e = e + y
            r = r + (y[su[0]] - y[su[1]])
        sumse, flat = sumse + e, flat + r
        lanes_p = [np.zeros(len(lo)) for _ in range(LANES)]
        lanes_q = [np.zeros(len(lo)) for _ in range(LANES)]
        for t, c0 in enumerate(range(0, d, TILE)):
            p, q = np.zeros(len(lo)), np.zeros(len(lo))
            for y in block:                                             # ascending samples, then ascending components of the tile
                for c in range(c0, min(c0 + TILE, d)):
                    a, b = y[lo, c], y[hi, c]
                    p = fma(w[c] * a, b, p)
                    if differences:
                        dd = a - b
                        q = fma(w[c] * dd, dd, q)
            lanes_p[t % LANES] = lanes_p[t % LANES] + p
            lanes_q[t % LANES] = lanes_q[t % LANES] + q
        pc, qc = pc + tree(lanes_p), qc + tree(lanes_q)
    sumsc, sumsd2 = np.zeros((L, L)), np.zeros((L, L))
    sumsc[lo, hi] = pc
    sumsc[hi, lo] = pc
    off = lo < hi
    sumsd2[lo[off], hi[off]] = qc[off]
    return (sumse, sumsc, flat, sumsd2) if differences else (sumse, sumsc, None, None)


def stats_ld(values, w):
    """(sumse [L, d], sumsc [L, L], sumsd1 [L, L, d], sumsd2 [L, L]) in long double, the difference sums at i < j, else 0; and the
    sums of the absolute values of the same terms"""
    Y, w = np.asarray(values, dtype=np.float64).astype(LD), np.asarray(w, dtype=np.float64).astype(LD)
    L = Y.shape[1]
    upper = np.triu(np.ones((L, L)), 1).astype(LD)
    D = Y[:, :, None, :] - Y[:, None, :, :]
    sums = (Y.sum(axis=0), np.einsum("sic,c,sjc->ij", Y, w, Y), D.sum(axis=0) * upper[:, :, None], np.einsum("sijc,c,sijc->ij", D, w, D) * upper)
    A, B = np.abs(Y), np.abs(D)
    mags = (A.sum(axis=0), np.einsum("sic,c,sjc->ij", A, w, A), B.sum(axis=0) * upper[:, :, None], np.einsum("sijc,c,sijc->ij", B, w, B) * upper)
    return sums, mags


def sum_bounds(values, w):
    """per entry of the four sums: n u sum|terms| with n = N d terms at most and the factor 4 of pilot_ref.cov_bound (two
    summations in different orders, and the product w_c a rounded before the fma)"""
    Y = np.asarray(values)
    n = Y.shape[0] * Y.shape[2]
    return tuple(4 * n * U * np.asarray(m, dtype=np.float64) for m in stats_ld(values, w)[1])


def cov_bound(values, w, N):
    """pilot_ref.cov_bound for a field: per entry 4 n u (sum|<y_i, y_j>| / N + <sum|y_i|, sum|y_j|> / N^2), n = N d, and the
    analogous bound for the difference variances [L, L]"""
    Y = np.asarray(values)
    n = Y.shape[0] * Y.shape[2]
    ae, ac, ad1, ad2 = (np.asarray(m, dtype=np.float64) for m in stats_ld(values, w)[1])
    w = np.asarray(w, dtype=np.float64)
    return (4 * n * U * (ac / N + np.einsum("ic,c,jc->ij", ae, w, ae) / N**2),
            4 * n * U * (ad2 / N + np.einsum("ijc,c,ijc->ij", ad1, w, ad1) / N**2))


def field_statistics(values, w, differences=True):
    """stand-in for bluest_amd.fields.field_statistics: the long-double sums rounded to float64"""
    se, sc, d1, d2 = (np.asarray(a, dtype=np.float64) for a in stats_ld(values, w)[0])
    return (se, sc, d1, d2) if differences else (se, sc, None, None)


# ---- bluest_field_sums -----------------------------------------------------------------------------------------------------------
def segment_sums(values):
    """[N, L, d] -> [L, d] with the kernel's bits: steps 1-3 of Part 11 per (column, component)"""
    v = np.asarray(values, dtype=np.float64)
    N, L, d = v.shape
    return gsums_ref.segment_sums(v.reshape(1, N, L * d))[0].reshape(L, d)


def field_group_sums(values, weights=None, repeat_of=None, R=None, slab_bytes=None):
    """stand-in for bluest_amd.fields.field_group_sums with the same bits: sums per segment, and mu[r][c] = the fma chain over
    the columns of repeat r in ascending order from +0.0"""
    vals = [np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v, dtype=np.float64) for v in values]
    sums = [segment_sums(v) for v in vals]
    if weights is None:
        return sums
    d = vals[0].shape[2]
    weights = np.asarray(weights, dtype=np.float64)
    repeat_of = np.zeros(len(vals), dtype=np.int64) if repeat_of is None else np.asarray(repeat_of, dtype=np.int64)
    R = int(repeat_of[-1]) + 1 if R is None else int(R)
    mu = np.zeros((R, d))
    col = 0
    for s, sm in enumerate(sums):
        for j in range(sm.shape[0]):
            mu[repeat_of[s]] = fma(np.full(d, weights[col]), sm[j], mu[repeat_of[s]])
            col += 1
    return sums, mu


def segment_ld(values):
    """[L, d] in long double, and the sums of the absolute values"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    return Y.sum(axis=0), np.abs(Y).sum(axis=0)

"""numpy restatement of bluest_field_weighted_moments (include/bluest_hip.h, Part 15): every subtraction, fma and addition in the
order the header states, so the result has the kernel's bits; a data generator for which that restatement runs at numpy's speed;
the long-double sums and the rounding bounds the results are held to; and a stand-in for
bluest_amd.field_errors.field_weighted_moments made of them.

The exact fma (gsums_ref.fma, through Fraction) costs microseconds per term: `segment_moments(values, coef)` is for shapes of at
most about 10^5 terms N * L * d.  `segment_moments(values, coef, exact_products=True)` is for the data of `data26`: every product
coef_j * d_ij[c], every partial sum of the chain and every z are integers below 2^26 times one power of two per component, so
fma(a, b, q) is q + a * b with no rounding at all in the chain and a single one in q = fma(z, z, q), which numpy does at full
speed -- the ORDER of the additions, which is what the kernel is held to, still decides the bits, because sixteen squares of
26-bit numbers already need more than 53 bits."""
import numpy as np

import gsums_ref
from gsums_ref import CHUNK, CLASSES, CLASS_ROWS, LANES, LD, U

_fma = np.frompyfunc(gsums_ref.fma, 3, 1)


def shifted(values):
    """d = values - the first sample, one rounding per value: [N, L, d]"""
    values = np.asarray(values, dtype=np.float64)
    return values - values[:1] if values.shape[0] else values.copy()


def few_bits(x, bits=26):
    """every value of x has at most `bits` significant bits"""
    m, _ = np.frexp(np.asarray(x, dtype=np.float64))
    return bool(np.all(np.ldexp(m, bits) == np.rint(np.ldexp(m, bits))))


def data26(N, L, d, seed, signed=False):
    """(values [N, L, d], coef [L]) for exact_products=True.  coef_j = k_j 2^t_j with an integer k_j in 1..7 (with `signed`: of
    either sign, and one of them 0 when L > 2); values[i, j, c] = n_ijc 2^(s_c - t_j) with integers n: the samples lie in the upper
    half of [0, D] and the first one in the upper half of [-D, 0], so every shifted difference is a positive integer of the order
    D, where D = (2^26 - 1) // (2 sum_j |k_j|).  Every term, every partial sum of the chain and every z is then an integer below
    2^26 times 2^s_c; unsigned, z is of the order 2^25 and above, its square fills 51 bits and sixteen of them need more than 53."""
    rng = np.random.RandomState(seed)
    k = rng.randint(1, 8, size=L).astype(np.float64)
    if signed:
        k *= rng.choice([-1.0, 1.0], size=L)
        if L > 2:
            k[rng.randint(L)] = 0.0
    D = (2 ** 26 - 1) // (2 * int(np.abs(k).sum()) or 1)
    ints = np.rint(D * (0.5 + 0.5 * rng.rand(N, L, d)))
    ints[:1] = -np.rint(D * (0.5 + 0.5 * rng.rand(min(N, 1), L, d)))
    t = rng.randint(-8, 9, size=L)
    s = rng.randint(-30, -10, size=d)
    return ints * 2.0 ** (s[None, None, :] - t[None, :, None]), k * 2.0 ** t


def chains(values, coef, exact_products=False):
    """z [N, d]: from +0.0, z = fma(coef_j, d_ij[c], z) over j ascending"""
    dv = shifted(values)
    coef = np.asarray(coef, dtype=np.float64)
    z = np.zeros((dv.shape[0], dv.shape[2]))
    for j in range(dv.shape[1]):
        if exact_products:
            z = z + coef[j] * dv[:, j, :]
            assert few_bits(coef[j] * dv[:, j, :]) and few_bits(z), "these chains are not exact: use the fma through Fraction"
        else:
            z = _fma(coef[j], dv[:, j, :], z).astype(np.float64)
    return z


def chunk_squares(block, exact_products):
    """[rows <= 128, d] of z -> [d]: eight classes of sixteen consecutive rows, each q = fma(z, z, q) in ascending order from
    +0.0, joined as ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))"""
    rows, d = block.shape
    q = []
    for k in range(CLASSES):
        acc = np.zeros(d)
        for r in range(k * CLASS_ROWS, min((k + 1) * CLASS_ROWS, rows)):
            if exact_products:
                acc = acc + block[r] * block[r]
            else:
                acc = _fma(block[r], block[r], acc).astype(np.float64)
        q.append(acc)
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))


def segment_moments(values, coef, exact_products=False):
    """[N, L, d], [L] -> (zsum [d], zsq [d]) with the kernel's bits"""
    z = chains(values, coef, exact_products)
    N, d = z.shape
    zsum = gsums_ref.segment_sums(z[None])[0]
    p = [np.zeros(d) for _ in range(LANES)]
    for c, start in enumerate(range(0, N, CHUNK)):
        p[c % LANES] = p[c % LANES] + chunk_squares(z[start:start + CHUNK], exact_products)
    off = LANES // 2
    while off > 0:
        for l in range(off):
            p[l] = p[l] + p[l + off]
        off //= 2
    return zsum, p[0]


def field_weighted_moments(values, coef, slab_bytes=None, exact_products=False):
    """stand-in for bluest_amd.field_errors.field_weighted_moments with the same bits"""
    coef = np.asarray(coef, dtype=np.float64)
    out, col = [], 0
    for v in values:
        v = np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v, dtype=np.float64)
        zsum, zsq = segment_moments(v, coef[col:col + v.shape[1]], exact_products)
        out.append((v.shape[0], zsum, zsq))
        col += v.shape[1]
    return out


def moments_ld(values, coef):
    """from the kernel's d (float64) in long double: (sum_i z_i [d], sum_i z_i^2 [d], bound of zsum [d], bound of zsq [d]) with
    z_i = sum_j coef_j d_ij.

    The bounds, with u = 2^-53 and A_i = sum_j |coef_j d_ij| >= |z_i|.  The chain of L fmas rounds once per step, so the computed
    z^_i is off by at most g_L A_i, g_n = n u / (1 - n u) (the product inside an fma is not rounded).  Adding the N numbers z^_i in
    any order with one rounding per addition is off by at most g_(N-1) sum_i |z^_i| <= g_N (1 + g_L) sum_i A_i.  Together
        |zsum^ - sum_i z_i| <= (g_L + g_N (1 + g_L)) sum_i A_i,    about (L + N) u sum_i A_i.
    For the squares |z^_i^2 - z_i^2| = |z^_i - z_i| |z^_i + z_i| <= g_L (2 + g_L) A_i^2, and the N fmas q = fma(z^, z^, q) round
    once each: g_N sum_i z^_i^2 <= g_N (1 + g_L)^2 sum_i A_i^2.  Together
        |zsq^ - sum_i z_i^2| <= about (2 L + N) u sum_i A_i^2.
    The tests allow TWICE these first-order terms, 2 (L + N) u sum A and 2 (2 L + N) u sum A^2, the convention of
    moments_ref.moments_ld: the factor covers the second-order terms (L, N <= 10^5: g below 2^-36) and the 2^-64 relative error of
    a long-double product or sum of this reference itself."""
    dv = shifted(values).astype(LD)
    coef = np.asarray(coef, dtype=np.float64).astype(LD)
    N, L, _ = dv.shape
    terms = coef[None, :, None] * dv
    z, A = terms.sum(axis=1), np.abs(terms).sum(axis=1)
    return (z.sum(axis=0), (z * z).sum(axis=0), 2 * (L + N) * U * A.sum(axis=0), 2 * (2 * L + N) * U * (A * A).sum(axis=0))


def variance_of(N, zsum, zsq):
    """the unbiased variance of z from its sums (the shift drops out); NaN where N < 2"""
    if N < 2:
        return np.full(np.shape(zsum), np.nan)
    return (zsq - zsum * zsum / N) / (N - 1)

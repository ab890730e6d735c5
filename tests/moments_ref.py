"""numpy restatement of bluest_group_moments (include/bluest_hip.h, Part 13): every subtraction, addition and fma in the order the
header states, so the result has the kernel's bits; the long-double sums of d and d d' and the rounding bound the results are held
to; and a stand-in for bluest_amd.moments.group_moments made of them.

The exact fma (gsums_ref.fma, through Fraction) costs microseconds per term: `segment_moments(values)` is for shapes of at most
about 10^5 terms n_out * N * L (L + 1) / 2.  `segment_moments(values, exact_products=True)` is for data whose products d_j d_k
are exactly representable (every d has at most 26 significant bits: `few_bits`, `data26`): fma(a, b, q) is then q + a * b with
its single rounding, which numpy does at full speed -- the ORDER of the additions, which is what the kernel is held to, still
decides the bits, because the sums of such products need more than 53 bits."""
import numpy as np

import gsums_ref
from gsums_ref import CHUNK, CLASSES, CLASS_ROWS, LANES, LD, U

_fma = np.frompyfunc(gsums_ref.fma, 3, 1)


def shifted(values):
    """d = values - the first sample, one rounding per value: [n_out, N, L]"""
    values = np.asarray(values, dtype=np.float64)
    return values - values[:, :1, :] if values.shape[1] else values.copy()


def few_bits(d, bits=26):
    """every value of d has at most `bits` significant bits: the product of two of them is exact in float64"""
    m, _ = np.frexp(np.asarray(d, dtype=np.float64))
    return bool(np.all(np.ldexp(m, bits) == np.rint(np.ldexp(m, bits))))


def data26(n_out, N, L, seed):
    """values whose shifted differences have at most 26 significant bits: column j is an integer below 2^24 in magnitude times
    2^s_j, so d is an integer below 2^25 times 2^s_j.  The samples lie around +2^23 and the first one around -2^23: every d is
    then of the order 2^24.5, the products fill their 52 bits and sixteen of them already need more than 53"""
    rng = np.random.RandomState(seed)
    ints = np.clip(np.rint(2.0 ** 23 + 2.0 ** 21 * rng.randn(n_out, N, L)), 0, 2.0 ** 24 - 1)
    ints[:, :1, :] = -np.clip(np.rint(2.0 ** 23 + 2.0 ** 21 * np.abs(rng.randn(n_out, min(N, 1), L))), 0, 2.0 ** 24 - 1)
    return ints * 2.0 ** rng.randint(-30, -10, size=L)


def chunk_products(block, exact_products):
    """[n_out, rows <= 128, L] of d -> [n_out, P]: per pair j <= k (row-major) eight classes of sixteen consecutive rows, each
    q = fma(d_j, d_k, q) in ascending order from +0.0, joined as ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))"""
    n_out, rows, L = block.shape
    j, k = np.triu_indices(L)
    q = []
    for c in range(CLASSES):
        acc = np.zeros((n_out, len(j)))
        for r in range(c * CLASS_ROWS, min((c + 1) * CLASS_ROWS, rows)):
            if exact_products:
                acc = acc + block[:, r, j] * block[:, r, k]
            else:
                acc = _fma(block[:, r, j], block[:, r, k], acc).astype(np.float64)
        q.append(acc)
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))


def segment_moments(values, exact_products=False):
    """[n_out, N, L] -> (first [n_out, L], second [n_out, P] packed as Part 13 packs it) with the kernel's bits"""
    d = shifted(values)
    n_out, N, L = d.shape
    if exact_products:
        assert few_bits(d), "the products of these values are not exact: use the fma through Fraction"
    first = gsums_ref.segment_sums(d)
    p = [np.zeros((n_out, L * (L + 1) // 2)) for _ in range(LANES)]
    for c, start in enumerate(range(0, N, CHUNK)):
        p[c % LANES] = p[c % LANES] + chunk_products(d[:, start:start + CHUNK, :], exact_products)
    off = LANES // 2
    while off > 0:
        for l in range(off):
            p[l] = p[l] + p[l + off]
        off //= 2
    return first, p[0]


def unpack(second, L):
    """[n_out, P] -> [n_out, L, L] full and symmetric"""
    j, k = np.triu_indices(L)
    full = np.zeros((second.shape[0], L, L))
    full[:, j, k] = second
    full[:, k, j] = second
    return full


def group_moments(values, slab_bytes=None, exact_products=False):
    """stand-in for bluest_amd.moments.group_moments with the same bits"""
    out = []
    for v in values:
        v = np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v, dtype=np.float64)
        first, second = segment_moments(v, exact_products)
        out.append((v.shape[1], first, unpack(second, v.shape[2])))
    return out


def moments_ld(values):
    """from the kernel's d (float64) in long double: (sum d [n_out, L], sum d d' [n_out, P], sum |d| and sum |d_j d_k|, the
    quantities the rounding bounds are stated in).  Adding n numbers in any order with one rounding per addition is off by at
    most (n - 1) u / (1 - (n - 1) u) times the sum of their absolute values; the fma adds no rounding of the product.  The tests
    allow 2 N u sum|.|, the bound tests/test_gpu_group_sums.py holds the column sums to; a long-double product of two float64
    numbers is itself off by 2^-64 relatively, which that factor of two covers."""
    d = shifted(values).astype(LD)
    j, k = np.triu_indices(d.shape[2])
    prod = d[:, :, j] * d[:, :, k]
    return d.sum(axis=1), prod.sum(axis=1), np.abs(d).sum(axis=1), np.abs(prod).sum(axis=1)


def covariance_ld(values):
    """the unbiased sample covariance [n_out, L, L] of the values themselves, two passes in long double"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    D = Y - Y.mean(axis=1, keepdims=True)
    return np.einsum("nij,nik->njk", D, D) / (Y.shape[1] - 1)

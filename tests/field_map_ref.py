"""Part 18 of include/bluest_hip.h restated in numpy, chain by chain: out[s, l, r] = row r of operator l applied to sample s of
values[l].  The entries of a row in their stored order, cut into strips of STRIP = 512; per strip p = fma(data[k], y[s, idx[k]], p)
from +0.0 in ascending k; a row of at most one strip is that chain, a longer one the strips' values added in ascending order
from +0.0; an empty row +0.0; None = identity, the value's bits.

The fma is exact (gsums_ref.fma, through Fraction) for general finite data.  With exact_products=True the caller states that
every product data[k] * y is exact in float64 (coefficients and finite values of at most 26 significant bits, few_bits), so
p + a * b has fma's one rounding; this path is vectorised over the samples and carries NaN / Inf as the device does (0 * NaN and
0 * Inf are NaN with or without the fused rounding)."""
import numpy as np

from gsums_ref import fma, same_bits  # noqa: F401  (same_bits: for the tests that import this module)

STRIP = 512
U = 2.0 ** -53
LD = np.longdouble


def few_bits(x, bits=26):
    """every finite value of x has at most `bits` significant bits"""
    x = np.asarray(x, dtype=np.float64)
    m, _ = np.frexp(x[np.isfinite(x)])
    return bool(np.all(np.ldexp(m, bits) == np.rint(np.ldexp(m, bits))))


def triple(op):
    """(indptr, indices, data, (q, d)) of a FieldOperator or of such a tuple"""
    if hasattr(op, "csr"):
        return tuple(op.csr()) + (tuple(op.shape),)
    indptr, indices, data, shape = op
    return np.asarray(indptr, dtype=np.int64), np.asarray(indices, dtype=np.int64), np.asarray(data, dtype=np.float64), tuple(shape)


def _chain(data, idx, y, ks, exact_products):
    """[N]: the fma chain over the entries ks of a row, from +0.0"""
    p = np.zeros(y.shape[0])
    for k in ks:
        a, b = float(data[k]), y[:, idx[k]]
        if exact_products:
            with np.errstate(invalid="ignore", over="ignore"):
                p = p + a * b
        else:
            p = np.array([fma(a, float(b[s]), float(p[s])) for s in range(len(p))])
    return p


def apply(op, y, exact_products=False):
    """[N, q] from y [N, d]"""
    indptr, idx, data, (q, d) = triple(op)
    y = np.asarray(y, dtype=np.float64)
    assert y.ndim == 2 and y.shape[1] == d
    if exact_products:
        assert few_bits(data) and few_bits(y), "exact_products needs coefficients and values of at most 26 significant bits"
    else:
        assert np.all(np.isfinite(y)), "the exact fma takes finite values: use exact_products for NaN / Inf"
    out = np.zeros((y.shape[0], q))
    for r in range(q):
        a, b = int(indptr[r]), int(indptr[r + 1])
        if b - a <= STRIP:
            out[:, r] = _chain(data, idx, y, range(a, b), exact_products)
        else:
            total = np.zeros(y.shape[0])
            for k0 in range(a, b, STRIP):
                with np.errstate(invalid="ignore", over="ignore"):
                    total = total + _chain(data, idx, y, range(k0, min(k0 + STRIP, b)), exact_products)
            out[:, r] = total
    return out


def map_fields(values, operators, exact_products=False, **_):
    """stand-in for bluest_amd.field_maps.map_fields with the same bits: a numpy array [N, L, q]"""
    values = [np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v, dtype=np.float64) for v in values]
    planes = [v.copy() if op is None else apply(op, v, exact_products) for v, op in zip(values, operators)]
    return np.ascontiguousarray(np.stack(planes, axis=1))


def dense(op):
    """the matrix [q, d] in long double; a column that occurs twice in a row adds up"""
    indptr, idx, data, (q, d) = triple(op)
    B = np.zeros((q, d), dtype=LD)
    for r in range(q):
        for k in range(int(indptr[r]), int(indptr[r + 1])):
            B[r, idx[k]] += LD(data[k])
    return B


def self_check(op, y, exact_products=False):
    """the restatement against B @ y in long double: a chain of n fmas (and the additions of its strips: fewer than n) differs
    from the exact row sum by at most gamma_n sum_k |a_k y_k| <= 1.01 (n + 1) u sum_k |a_k| |y_k|; the long-double product itself
    is exact to 2^-64 of the same sum per term, far inside the margin.  Returns the largest error / bound (0 for exact rows)."""
    indptr, idx, data, (q, d) = triple(op)
    y = np.asarray(y, dtype=np.float64)
    got = apply(op, y, exact_products)
    want = y.astype(LD) @ dense(op).T
    mag = np.abs(y).astype(LD) @ np.abs(dense_abs(op)).T
    n = np.diff(indptr).astype(np.float64)
    bound = (1.01 * (n + 1) * U)[None, :] * mag.astype(np.float64)
    err = np.abs(got.astype(LD) - want).astype(np.float64)
    assert np.all(err <= bound), float((err - bound).max())
    return float(np.max(err[bound > 0] / bound[bound > 0])) if np.any(bound > 0) else 0.0


def dense_abs(op):
    """sum_k |a_k| per (row, column): the magnitudes the rounding bound is stated in"""
    indptr, idx, data, shape = triple(op)
    return dense((indptr, idx, np.abs(data), shape))


# ---- operators for the tests ---------------------------------------------------------------------------------------------------------
def interpolation_1d(n_from, n_to):
    """linear interpolation from n_from to n_to equally spaced nodes of [0, 1] as a CSR tuple (n_to x n_from): two entries per
    row with columns ascending, one where a node of the target is a node of the source"""
    indptr, indices, data = [0], [], []
    for r in range(n_to):
        x = r / (n_to - 1) * (n_from - 1)
        j = min(int(np.floor(x)), n_from - 2)
        t = x - j
        for c, a in ((j, 1.0 - t), (j + 1, t)):
            if a != 0.0:
                indices.append(c)
                data.append(a)
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data), (n_to, n_from)


def random_operator(rng, q, d, lengths, bits=26):
    """a CSR tuple whose row r has lengths[r % len(lengths)] entries (capped by nothing: columns repeat where a row is longer
    than d), columns in random order, coefficients k 2^e with |k| < 2^10 (some of them 0): `bits`-bit products with data26"""
    indptr, indices, data = [0], [], []
    for r in range(q):
        n = int(lengths[r % len(lengths)])
        indices.extend(rng.randint(0, d, size=n).tolist())
        k = rng.randint(-1023, 1024, size=n).astype(np.float64)
        data.extend((k * 2.0 ** rng.randint(-6, 7, size=n)).tolist())
        indptr.append(len(indices))
    return np.array(indptr, dtype=np.int64), np.array(indices, dtype=np.int32), np.array(data), (q, d)


def data26(rng, N, d):
    """values [N, d] of at most 16 significant bits and mixed magnitudes: with random_operator's coefficients every product is
    exact, while the sums round"""
    return rng.randint(-32767, 32768, size=(N, d)).astype(np.float64) * 2.0 ** rng.randint(-20, 21, size=(N, d))

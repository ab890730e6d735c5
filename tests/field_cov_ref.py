"""numpy restatement of bluest_field_group_moments (include/bluest_hip.h, Part 16): every subtraction, product, fma and addition
in the order the header states, so the result has the kernel's bits; the long-double sums and the rounding bounds the results are
held to; and a stand-in for bluest_amd.field_covariances.field_group_moments made of them.

The exact fma (gsums_ref.fma, through Fraction) costs microseconds per term: `segment_moments(values, w)` is for shapes of at most
a few 10^5 terms N * L (L + 1) / 2 * d.  `segment_moments(values, w, exact_products=True)` is for the data of
field_moments_ref.data26 with weights that are powers of two or zero (`weights_pow2`): every shifted value has at most 26
significant bits, w_c * a is exact and so is (w_c * a) * b, so fma(w_c * a, b, q) is q + (w_c * a) * b with its single rounding,
which numpy does at full speed -- the ORDER of the additions, which is what the kernel is held to, still decides the bits, because
the sums of such products need more than 53 bits.  The first moments f fill their 53 bits, so `cross` has no such shortcut; with
exact_products its fma is the C library's (correctly rounded as well, and several times faster than Fraction's;
tests/test_field_covariances_host.py holds the two against each other)."""
import ctypes
import ctypes.util

import numpy as np

import gsums_ref
from field_moments_ref import few_bits, shifted
from gsums_ref import CHUNK, CLASSES, CLASS_ROWS, LANES, LD, U

TILE = 8
_fma = np.frompyfunc(gsums_ref.fma, 3, 1)
_libm = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_libm.fma.restype = ctypes.c_double
_libm.fma.argtypes = [ctypes.c_double] * 3
_fma_c = np.frompyfunc(_libm.fma, 3, 1)


def weights_pow2(d, seed, zeros=True):
    """[d] weights 2^e, e in -3..3, about one in five of them 0 (not the first)"""
    rng = np.random.RandomState(seed)
    w = 2.0 ** rng.randint(-3, 4, size=d)
    if zeros and d > 1:
        w[1:][rng.rand(d - 1) < 0.2] = 0.0
    return w


def class_tree(q):
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))


def lane_tree(values):
    """the join of Part 11, step 3, over axis 0: lane l adds the entries l, l + 64, ... in ascending order from +0.0, then for
    off = 32 .. 1 lane l < off takes p[l] + p[l + off]; the result is lane 0's"""
    p = [np.zeros(values.shape[1:]) for _ in range(LANES)]
    for i in range(values.shape[0]):
        p[i % LANES] = p[i % LANES] + values[i]
    off = LANES // 2
    while off > 0:
        for l in range(off):
            p[l] = p[l] + p[l + off]
        off //= 2
    return p[0]


def tiled(x, d):
    """[..., d] -> [..., ntiles, 8], the last tile filled with +0.0.  With w = +0.0 there as well the terms of the filling are
    fma(+0.0 * +0.0, +0.0, q) = q + 0.0, which leaves every q of these chains alone: they start from +0.0 and are never -0.0."""
    ntiles = (d + TILE - 1) // TILE
    out = np.zeros(x.shape[:-1] + (ntiles * TILE,))
    out[..., :d] = x
    return out.reshape(x.shape[:-1] + (ntiles, TILE))


def chunk_second(block, wt, j, k, exact_products, width=TILE):
    """[rows <= 128, L, ntiles, 8] of d, w [ntiles, 8] -> [P]: per pair and tile eight classes of sixteen consecutive rows, each
    q = fma(w_c * a, b, q) over the rows in ascending order and inside a row over the tile's components in ascending order, from
    +0.0; the classes join in the tree, the tiles in the lane sums and the tree of Part 12"""
    rows, ntiles = block.shape[0], block.shape[2]
    q = []
    for cls in range(CLASSES):
        acc = np.zeros((ntiles, len(j)))
        for r in range(cls * CLASS_ROWS, min((cls + 1) * CLASS_ROWS, rows)):
            for c in range(min(TILE, width)):                                # (the filling of a lone short tile changes no bit)
                a, b = block[r, j, :, c].T, block[r, k, :, c].T              # [ntiles, P]
                wa = wt[:, c, None] * a
                if exact_products:
                    acc = acc + wa * b
                else:
                    acc = _fma(wa, b, acc).astype(np.float64)
        q.append(acc)
    return lane_tree(class_tree(q))


def cross_of(f, w, exact_products=False):
    """f [L, d], w [d] -> [P]: per pair j <= k and tile x = fma(w_c * f_j[c], f_k[c], x) over the tile's components in ascending
    order from +0.0; the tiles join in the lane sums and the tree"""
    L, d = f.shape
    j, k = np.triu_indices(L)
    ft, wt = tiled(f, d), tiled(np.asarray(w, dtype=np.float64), d)
    x = np.zeros((ft.shape[1], len(j)))
    if f.any():
        fma = _fma_c if exact_products else _fma
        for c in range(TILE):
            x = fma(wt[:, c, None] * ft[j, :, c].T, ft[k, :, c].T, x).astype(np.float64)
    return lane_tree(x)


def segment_moments(values, w, exact_products=False):
    """[N, L, d], [d] -> (first [L, d], second [P], cross [P]) with the kernel's bits, P packed as Part 13 packs it"""
    dv = shifted(values)
    w = np.asarray(w, dtype=np.float64)
    N, L, d = dv.shape
    if exact_products:
        assert few_bits(dv) and few_bits(w, 1), "the products of these values are not exact: use the fma through Fraction"
    first = gsums_ref.segment_sums(dv.reshape(1, N, L * d))[0].reshape(L, d)
    j, k = np.triu_indices(L)
    dt, wt = tiled(dv, d), tiled(w, d)
    chunks = [chunk_second(dt[start:start + CHUNK], wt, j, k, exact_products, d) for start in range(0, N, CHUNK)]
    second = lane_tree(np.array(chunks)) if chunks else np.zeros(len(j))
    return first, second, cross_of(first, w, exact_products)


def unpack(packed, L):
    """[P] -> [L, L] full and symmetric"""
    j, k = np.triu_indices(L)
    full = np.zeros((L, L))
    full[j, k] = packed
    full[k, j] = packed
    return full


def field_group_moments(values, w, with_first=False, slab_bytes=None, exact_products=False):
    """stand-in for bluest_amd.field_covariances.field_group_moments with the same bits"""
    out = []
    for v in values:
        v = np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v, dtype=np.float64)
        first, second, cross = segment_moments(v, w, exact_products)
        L = v.shape[1]
        out.append((v.shape[0], unpack(second, L), unpack(cross, L)) + ((first,) if with_first else ()))
    return out


def moments_ld(values, w):
    """from the kernel's d (float64) in long double: (f [L, d], second [P], cross [P], sum_i |d| [L, d], sum |w a b| [P],
    sum_c |w_c| F_j[c] F_k[c] [P] with F = sum_i |d|), the quantities the rounding bounds are stated in.
    second adds N d' terms (d' = d filled up to whole tiles) with one rounding each, the product w_c * a adds one more per term:
    |second^ - second| <= about (N d + 8 + 1) u sum |w a b| to first order; the tests allow 2 (N d + 9) u sum |w a b|.
    f_j[c] is off by at most about N u F_j[c], so a term of cross is off by (2 N + 1) u |w| F_j F_k, and the d additions add
    d u of the sum: the tests allow 2 (2 N + d + 9) u sum_c |w_c| F_j[c] F_k[c].  The factor 2 covers the second-order terms and
    the 2^-64 relative error of a long-double operation of this reference itself, the convention of moments_ref.moments_ld."""
    dv = shifted(values).astype(LD)
    wl = np.asarray(w, dtype=np.float64).astype(LD)
    j, k = np.triu_indices(dv.shape[1])
    f, F = dv.sum(axis=0), np.abs(dv).sum(axis=0)
    prod = dv[:, j, :] * dv[:, k, :] * wl
    return (f, prod.sum(axis=(0, 2)), (f[j] * f[k] * wl).sum(axis=1), F, np.abs(prod).sum(axis=(0, 2)), (F[j] * F[k] * wl).sum(axis=1))


def covariance_ld(values, w):
    """the unbiased sample covariance [L, L] of the values themselves in the inner product, two passes in long double"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    D = Y - Y.mean(axis=0, keepdims=True)
    return np.einsum("ijc,c,ikc->jk", D, np.asarray(w, dtype=np.float64).astype(LD), D) / (Y.shape[0] - 1)


def covariance_of(N, second, cross):
    if N < 2:
        return np.full(np.shape(second), np.nan)
    return (second - cross / N) / (N - 1)

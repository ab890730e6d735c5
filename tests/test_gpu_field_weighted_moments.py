"""
GPU tests of bluest_field_weighted_moments (include/bluest_hip.h Part 15, csrc/field_moments.hip) at its ABI: exact on small
integers; the bits of the numpy restatement of the documented order (tests/field_moments_ref.py) at every chunk edge, at every
(L, d) at which the launch takes another shape and where the fold's lanes wrap; inside the rounding bound of a long-double sum;
independent of the other segments of the call, of host or device memory, of the alignment of the base and of the slab size;
stable at a mean of 1e8; anchored to bluest_group_moments and to bluest_field_sums; strict about its arguments.

Two kinds of data.  `general`: any float64, held to the restatement through the exact fma (Fraction), so only at shapes of at
most a few 10^4 terms.  `field_moments_ref.data26`: values for which the chains are exact, so that the restatement runs at numpy's
speed at any shape while the order of the additions still decides the bits.

The launch shapes (csrc/field_moments.hip): d >= 64 reads memory along c; below, sub-blocks of sb rows are staged in LDS, sb the
largest power of two <= 128 with sb ((L d | 1) + d) + 16 d <= 4096.  `sub_rows` restates that rule.  The break between two values of
sb moves with both L and d; BREAKS holds, for d = 1, 2, 7, 15 and 63, the two group sizes on either side of every break there is
along L (every pair of neighbouring sb from 128 | 64 down to 2 | 1 at least once), and DS holds both sides of d = 64.  The wide
shape gives every class of a chunk a workgroup of its own where 64 <= d < 1024 and L >= 16: SPLIT_EDGES holds both sides of both.
"""
import ctypes

import numpy as np
import pytest

import field_moments_ref as ref
import gsums_ref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

CHUNK = 128
COUNTS = (0, 1, 2, 15, 16, 17, 127, 128, 129, 8191, 8192, 8193)
LS = (1, 2, 3, 5, 32, 64)
DS = (1, 2, 7, 8, 9, 63, 64, 65, 257)
# both sides of every break of sb: (L, d) -> sb
BREAKS = {(29, 1): 128, (30, 1): 64, (61, 1): 64, (62, 1): 32,
          (14, 2): 128, (15, 2): 64, (30, 2): 64, (31, 2): 32, (62, 2): 32, (63, 2): 16,
          (3, 7): 128, (4, 7): 64, (7, 7): 64, (8, 7): 32, (16, 7): 32, (17, 7): 16, (34, 7): 16, (35, 7): 8,
          (1, 15): 128, (2, 15): 64, (3, 15): 64, (4, 15): 32, (7, 15): 32, (8, 15): 16, (15, 15): 16, (16, 15): 8, (31, 15): 8,
          (32, 15): 4, (63, 15): 4, (64, 15): 2,
          (2, 63): 16, (3, 63): 8, (5, 63): 8, (6, 63): 4, (11, 63): 4, (12, 63): 2, (23, 63): 2, (24, 63): 1, (64, 63): 1}
SPLIT_EDGES = [(15, 64), (16, 64), (15, 1023), (16, 1023), (16, 1024)]    # a workgroup per class where 64 <= d < 1024 and L >= 16
SHAPES = sorted(set((L, d) for L in LS for d in DS) | set(BREAKS) | set(SPLIT_EDGES))
ERR_ARG = 1
U = gsums_ref.U
LD = np.longdouble


def sub_rows(L, d):
    """rows per staged sub-block; 0: the wide shape"""
    if d >= 64:
        return 0
    sb = CHUNK
    while sb > 1 and sb * ((L * d | 1) + d) + 16 * d > 4096:
        sb //= 2
    return sb


def counts_for(L, d):
    """the large counts only where three segments of them stay below about 64 MB"""
    return [N for N in COUNTS if N <= 129 or L * d <= 320]


def general(N, L, d, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models"""
    rng = np.random.RandomState(seed)
    return 1.5 + 10.0 ** rng.uniform(-3, 3, L)[None, :, None] * rng.randn(N, L, d)


def general_coef(L, seed):
    return np.random.RandomState(seed).randn(L) * 10.0 ** np.random.RandomState(seed + 1).uniform(-2, 2, L)


def raw(segs, coef, override=None):
    """the raw call on a list of host arrays / CUDA tensors [N, L, d]: (rc, zsum [S, d], zsq [S, d])"""
    from bluest_amd import _lib
    S, d = len(segs), int(segs[0].shape[2])
    counts = np.array([int(v.shape[0]) for v in segs], dtype=np.int64)
    sizes = np.array([int(v.shape[1]) for v in segs], dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(v) if v.shape[0] > 0 else None for v in segs])
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64))
    assert coef.shape == (int(sizes.sum()),)
    zsum, zsq = np.full((S, d), -7.0), np.full((S, d), -7.0)
    args = dict(S=S, d=d, counts=_lib.ptr(counts), sizes=_lib.ptr(sizes), values=ctypes.cast(ptrs, ctypes.c_void_p),
                coef=_lib.ptr(coef), zsum=_lib.ptr(zsum), zsq=_lib.ptr(zsq), stream=None)
    for k, v in (override or {}).items():                              # an argument of the call replaced as it is
        args[k] = _lib.ptr(v) if isinstance(v, np.ndarray) else v
    rc = _lib.lib().bluest_field_weighted_moments(*[args[k] for k in ("S", "d", "counts", "sizes", "values", "coef", "zsum", "zsq", "stream")])
    return rc, zsum, zsq


def same(got, want):
    return same_bits(got[0], want[0]) and same_bits(got[1], want[1])


def test_the_shapes_cover_every_launch_shape():
    assert all(sub_rows(L, d) == sb for (L, d), sb in BREAKS.items())
    assert {sub_rows(L, d) for L, d in SHAPES} == {0, 1, 2, 4, 8, 16, 32, 64, 128}
    assert sub_rows(64, 63) == 1 and sub_rows(1, 63) > 0 and sub_rows(1, 64) == 0


@pytest.mark.parametrize("L,d", SHAPES)
def test_small_integers_are_summed_exactly(L, d):
    """values below 8 and coefficients below 4 in magnitude: every z is an integer below 2^12, every sum below 2^53, so any order
    gives the same answer"""
    rng = np.random.RandomState(100 * L + d)
    segs = [rng.randint(-7, 8, size=(N, L, d)).astype(np.float64) for N in counts_for(L, d)]
    coef = rng.randint(-3, 4, size=L * len(segs)).astype(np.float64)
    rc, zsum, zsq = raw(segs, coef)
    assert rc == 0
    for s, v in enumerate(segs):
        z = np.einsum("j,ijc->ic", coef[s * L:(s + 1) * L], v - v[:1] if v.shape[0] else v)
        assert np.array_equal(zsum[s], z.sum(axis=0)) and np.array_equal(zsq[s], (z * z).sum(axis=0)), (L, d, v.shape[0])
        if v.shape[0] < 2:                                              # no sample, or d = 0: +0.0 everywhere
            assert not np.signbit(zsum[s]).any() and not np.signbit(zsq[s]).any() and (zsum[s] == 0).all() and (zsq[s] == 0).all()


@pytest.mark.parametrize("L,d", SHAPES)
def test_bits_of_the_restatement_at_every_chunk_edge(L, d):
    """data26 at every count, alternately with coefficients of one sign and of both (one of them zero), and general data through
    the exact fma at the counts where the shape is small enough for it"""
    plain = [ref.data26(N, L, d, 13 * L + 7 * d + N, signed=bool(i % 2)) for i, N in enumerate(counts_for(L, d))]
    slow = [(general(N, L, d, 17 * L + N), general_coef(L, N + d)) for N in (2, 17, 129) if N * L * d <= 20000]
    both = plain + slow
    rc, zsum, zsq = raw([v for v, _ in both], np.concatenate([c for _, c in both]))
    assert rc == 0
    for i, (v, c) in enumerate(both):
        assert same((zsum[i], zsq[i]), ref.segment_moments(v, c, exact_products=i < len(plain))), (L, d, v.shape[0], i < len(plain))


@pytest.mark.parametrize("L,d", [(3, 1), (64, 1), (5, 7), (3, 63), (2, 65), (1, 257), (16, 64)])
def test_more_chunks_than_fold_lanes(L, d):
    """64 and 65 chunks (8191, 8192, 8193 samples): the fold's lanes wrap; 130 chunks: a lane takes a third chunk.  (16, 64): the
    fold joins the eight class sums of every chunk itself; 65 chunks alone, 67 MB"""
    counts = ([8191, 8192, 8193] if L * d <= 320 else [8193]) + ([129 * CHUNK + 1] if L * d <= 64 else [])
    data = [ref.data26(N, L, d, L + d + N) for N in counts]
    rc, zsum, zsq = raw([v for v, _ in data], np.concatenate([c for _, c in data]))
    assert rc == 0
    for i, (v, c) in enumerate(data):
        assert same((zsum[i], zsq[i]), ref.segment_moments(v, c, exact_products=True)), (L, d, v.shape[0])


@pytest.mark.parametrize("N,L,d", [(8193, 5, 7), (300, 64, 63), (1000, 32, 9), (129, 3, 257), (2000, 64, 1), (700, 2, 64)])
def test_general_data_is_inside_the_long_double_bound(N, L, d):
    v, c = general(N, L, d, N + L), general_coef(L, d)
    rc, zsum, zsq = raw([v], c)
    assert rc == 0
    s1, s2, b1, b2 = ref.moments_ld(v, c)
    e1, e2 = np.abs(zsum[0].astype(LD) - s1), np.abs(zsq[0].astype(LD) - s2)
    print("largest error / bound: zsum", float((e1 / b1).max()), "zsq", float((e2 / b2).max()))
    assert (e1 <= b1).all() and (e2 <= b2).all()


@pytest.fixture(scope="module", params=[3, 70])
def pool(request):
    """41 ragged segments of data26 with d = 3 (staged, sb from 128 down to 8) or d = 70 (wide) and the restatement's moments of
    each, computed once: counts around every chunk edge, zero and one sample in the middle, every group size class"""
    d = request.param
    rng = np.random.RandomState(40 + d)
    sizes = [1, 2, 3, 5, 9, 10, 20, 21, 32, 42, 43, 63, 64] + rng.randint(1, 12, size=28).tolist()
    counts = [389, 5, 129, 0, 128, 17, 300, 1, 127, 16, 257, 200, 131] + rng.randint(1, 300, size=28).tolist()
    data = [ref.data26(N, L, d, 3000 + i, signed=bool(i % 2)) for i, (N, L) in enumerate(zip(counts, sizes))]
    segs, coefs = [v for v, _ in data], [c for _, c in data]
    return segs, coefs, [ref.segment_moments(v, c, exact_products=True) for v, c in data]


def test_forty_one_segments_host_and_device_mixed(pool):
    import torch
    segs, coefs, want = pool
    assert len(segs) == 41
    mixed = [torch.from_numpy(v).cuda() if i % 3 == 1 and v.shape[0] > 0 else v for i, v in enumerate(segs)]
    torch.cuda.synchronize()
    rc, zsum, zsq = raw(mixed, np.concatenate(coefs))
    assert rc == 0
    for i, w in enumerate(want):
        assert same((zsum[i], zsq[i]), w), (i, segs[i].shape)
    rc2, a2, b2 = raw(mixed, np.concatenate(coefs))
    assert rc2 == 0 and same_bits(a2, zsum) and same_bits(b2, zsq)
    for i, (v, c) in enumerate(zip(segs, coefs)):                       # and inside the rounding bound
        s1, s2, b1, b2 = ref.moments_ld(v, c)
        assert (np.abs(zsum[i].astype(LD) - s1) <= b1).all() and (np.abs(zsq[i].astype(LD) - s2) <= b2).all()


def test_a_segment_keeps_its_bits_alone_in_a_batch_on_the_device_and_at_another_base(pool):
    import torch
    segs, coefs, want = pool
    for i in (0, 2, 4, 6, 9, 11, 12):                                   # L = 1, 3, 9, 20, 42, 63, 64
        v, c = segs[i], coefs[i]
        rc, a, b = raw([v], c)
        assert rc == 0 and same((a[0], b[0]), want[i])
        others = [1, 8, 7]
        for order in ([i] + others, others + [i], others[:2] + [i] + others[2:]):
            rc, a, b = raw([segs[k] for k in order], np.concatenate([coefs[k] for k in order]))
            at = order.index(i)
            assert rc == 0 and same((a[at], b[at]), want[i])
        dev = torch.from_numpy(v).cuda()
        flat = torch.zeros(v.size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = torch.from_numpy(v).reshape(-1)
        shifted = flat[1:].reshape(v.shape)                             # 8- but not 16-byte aligned
        torch.cuda.synchronize()
        assert shifted.data_ptr() % 16 == 8 and dev.data_ptr() % 16 == 0
        for t in (dev, shifted):
            rc, a, b = raw([t], c)
            assert rc == 0 and same((a[0], b[0]), want[i])
        host = np.zeros(v.size + 1)
        host[1:] = v.reshape(-1)
        rc, a, b = raw([host[1:].reshape(v.shape)], c)                  # the same from the host
        assert rc == 0 and same((a[0], b[0]), want[i])


def test_a_tiny_slab_budget_gives_the_same_bits(pool):
    """the shift-row trap: under a budget of one chunk every later chunk of a host segment is staged without its first sample"""
    from bluest_amd import _lib, field_errors
    segs, coefs, want = pool
    d = segs[0].shape[2]
    big = [ref.data26(5 * CHUNK + 9, 7, d, 3), ref.data26(3, 4, d, 4), ref.data26(2 * CHUNK + 5, 30, d, 5, signed=True)]
    vals, coef = [v for v, _ in big], np.concatenate([c for _, c in big])
    want_big = [ref.segment_moments(v, c, exact_products=True) for v, c in big]
    rc, a, b = raw(vals, coef)
    assert rc == 0 and all(same((a[i], b[i]), w) for i, w in enumerate(want_big))
    lib, before = _lib.lib(), ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(1, ctypes.byref(before)) == 0 and before.value == 256 << 20
    try:
        rc1, a1, b1 = raw(vals, coef)                                   # room for one chunk of the widest segment
        assert lib.bluest_group_sums_slab(3 * CHUNK * 7 * d * 8 + 1000, None) == 0
        rc2, a2, b2 = raw(vals, coef)                                   # the first segment ends in the middle of a slab
        rc3, a3, b3 = raw(segs[:20], np.concatenate(coefs[:20]))
    finally:
        assert lib.bluest_group_sums_slab(before.value, None) == 0
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    assert same_bits(a1, a) and same_bits(b1, b) and same_bits(a2, a) and same_bits(b2, b)
    assert all(same((a3[i], b3[i]), w) for i, w in enumerate(want[:20]))
    py = field_errors.field_weighted_moments(vals, coef, slab_bytes=1)  # the Python entry sets the budget for its call only
    for (N, pa, pb), v, w in zip(py, vals, want_big):
        assert N == v.shape[0] and same((pa, pb), w)
    now = ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(0, ctypes.byref(now)) == 0 and now.value == before.value


@pytest.mark.parametrize("d", [5, 70])
def test_a_mean_of_1e8_keeps_nine_digits_where_the_raw_sums_keep_none(d):
    """values = 1e8 + N(0, 1): the variance of z from the shifted sums agrees with a two-pass long-double variance to 1e-9;
    sum z^2 - N zbar^2 in float64 on the same data does not"""
    from bluest_amd import field_errors
    rng = np.random.RandomState(8)
    N, L = 3000, 4
    v = 1e8 + rng.randn(N, L, d)
    c = np.array([0.7, -0.2, 0.4, 0.1])
    (_, zsum, zsq), = field_errors.field_weighted_moments([v], c)
    var = field_errors.variance_of(N, zsum, zsq)
    z = np.einsum("j,ijc->ic", c.astype(LD), v.astype(LD))
    want = ((z - z.mean(axis=0)) ** 2).sum(axis=0) / (N - 1)
    rel = (np.abs(var.astype(LD) - want) / want).astype(np.float64)
    z64 = np.einsum("j,ijc->ic", c, v)
    raw_var = ((z64 * z64).sum(axis=0) - N * z64.mean(axis=0) ** 2) / (N - 1)
    rel_raw = (np.abs(raw_var.astype(LD) - want) / want).astype(np.float64)
    print("shifted sums:", rel.max(), "raw float64 sums:", rel_raw.max())
    assert rel.max() <= 1e-9
    assert rel_raw.max() > 1e-9


@pytest.mark.parametrize("d", [1, 2, 7, 63, 64])
def test_the_two_anchors_against_group_moments(d):
    """one model with coefficient 1.0: z = d, so zsum is `first` and zsq the diagonal of `second` of bluest_group_moments on the
    same N x d values read as [n_out = 1, N, L = d], bit for bit"""
    from bluest_amd import moments
    segs = [general(N, 1, d, 5 * N + d) for N in (1, 2, 17, 129, 1000)]
    rc, zsum, zsq = raw(segs, np.ones(len(segs)))
    assert rc == 0
    got = moments.group_moments([np.ascontiguousarray(v[:, 0, :][None]) for v in segs])
    for s, (N, first, second) in enumerate(got):
        assert same_bits(zsum[s], first[0]) and same_bits(zsq[s], np.diagonal(second[0])), (d, N)


def test_the_sums_agree_with_field_sums():
    """sum_s (zsum_s + N_s sum_j coef_j a_j), a_j the first sample, is the estimator mu of bluest_field_sums with the same weights.
    Bound: the one of zsum (field_moments_ref.moments_ld), u sum |coef_j d_ij| for the rounding of the shift itself, and for mu
    2 (N + T) u sum_col |coef_col| sum_i |y| (N additions per column, then T fmas)."""
    from bluest_amd import fields
    d = 9
    data = [(general(N, L, d, N + L), general_coef(L, N)) for N, L in ((300, 3), (129, 5), (1, 2), (50, 1))]
    segs, coef = [v for v, _ in data], np.concatenate([c for _, c in data])
    rc, zsum, _ = raw(segs, coef)
    assert rc == 0
    _, mu = fields.field_group_sums(segs, weights=coef)
    lhs, bound, T, Nmax = np.zeros(d, dtype=LD), np.zeros(d, dtype=LD), len(coef), 300
    for s, (v, c) in enumerate(data):
        lhs += zsum[s].astype(LD) + v.shape[0] * (c.astype(LD)[:, None] * v[0].astype(LD)).sum(axis=0)
        A = np.abs(c.astype(LD)[None, :, None] * ref.shifted(v).astype(LD)).sum(axis=(0, 1))
        bound += ref.moments_ld(v, c)[2] + U * A + 2 * (Nmax + T) * U * (np.abs(c)[None, :, None] * np.abs(v)).sum(axis=(0, 1))
    err = np.abs(lhs - mu[0].astype(LD))
    print("largest error / bound:", float((err / bound).max()))
    assert (err <= bound).all()


@pytest.mark.parametrize("d", [3, 64])
def test_zero_coefficients(d):
    """a column with coefficient 0 leaves the chain as it is (fma(0, x, z) = z for finite x): the bits of the segment without that
    column; a segment whose coefficients are all 0 gives +0.0"""
    v, c = general(200, 4, d, 1), np.array([0.5, 0.0, -2.0, 0.0])
    rc, zsum, zsq = raw([v, v, np.ascontiguousarray(v[:, [0, 2], :])], np.concatenate([c, np.zeros(4), c[[0, 2]]]))
    assert rc == 0
    assert same((zsum[0], zsq[0]), (zsum[2], zsq[2])) and zsq[0].min() > 0
    assert (zsum[1] == 0).all() and (zsq[1] == 0).all() and not np.signbit(zsum[1]).any() and not np.signbit(zsq[1]).any()


@pytest.mark.parametrize("d", [3, 65])
def test_nan_and_inf_propagate(d):
    v = general(300, 3, d, 1)
    v[200, 1, 2] = np.nan
    w = general(40, 2, d, 2)
    w[7, 0, 1] = np.inf
    x = general(9, 2, d, 3)
    x[0, 1, 0] = np.inf                                                 # in the first sample: Inf - Inf = NaN in that component
    clean = general(50, 3, d, 4)
    coef = np.array([1.0, 2.0, -1.0, 0.5, 0.25, 1.0, 1.0, 0.3, -0.7, 0.2])
    rc, zsum, zsq = raw([v, w, x, clean], coef)
    assert rc == 0
    others = [c for c in range(d) if c != 2]
    assert np.isnan(zsum[0, 2]) and np.isnan(zsq[0, 2]) and np.isfinite(zsum[0, others]).all() and np.isfinite(zsq[0, others]).all()
    assert np.isposinf(zsum[1, 1]) and np.isposinf(zsq[1, 1]) and np.isfinite(zsum[1, [0, 2]]).all()
    assert np.isnan(zsum[2, 0]) and np.isnan(zsq[2, 0]) and np.isfinite(zsum[2, 1:]).all()
    assert same((zsum[3], zsq[3]), ref.segment_moments(clean, coef[7:]))    # the neighbours are untouched


def test_argument_errors():
    from bluest_amd import _lib
    lib = _lib.lib()
    a, b = np.ones((4, 3, 2)), 2 * np.ones((2, 2, 2))
    a[1:, 0, 0] = [2, 3, 4]
    coef = np.array([2.0, 1.0, 1.0, 1.0, 1.0])
    rc, zsum, zsq = raw([a, b], coef)
    assert rc == 0 and zsum.tolist() == [[12.0, 0.0], [0.0, 0.0]] and zsq.tolist() == [[56.0, 0.0], [0.0, 0.0]]
    i64, i32 = (lambda *x: np.array(x, dtype=np.int64)), (lambda *x: np.array(x, dtype=np.int32))
    odd = np.zeros(4 * 3 * 2 * 8 + 8, dtype=np.uint8)[4:4 + 192]       # a base that is not 8-byte aligned
    bad = {"S = 0": dict(S=0), "S < 0": dict(S=-1), "d = 0": dict(d=0), "d < 0": dict(d=-2),
           "counts": dict(counts=None), "sizes": dict(sizes=None), "values": dict(values=None), "coef": dict(coef=None),
           "zsum": dict(zsum=None), "zsq": dict(zsq=None), "size 0": dict(sizes=i32(3, 0)), "size 65": dict(sizes=i32(65, 2)),
           "negative count": dict(counts=i64(4, -1)), "nan coefficient": dict(coef=np.array([2.0, np.nan, 1.0, 1.0, 1.0])),
           "inf coefficient": dict(coef=np.array([2.0, 1.0, 1.0, 1.0, -np.inf])),
           "null segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(_lib.ptr(a), None), ctypes.c_void_p)),
           "misaligned segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(odd.ctypes.data, _lib.ptr(b)), ctypes.c_void_p))}
    assert odd.ctypes.data % 8 == 4
    for what, change in bad.items():
        rc, z1, z2 = raw([a, b], coef, override=change)
        assert rc == ERR_ARG, what
        assert len(lib.bluest_last_error()) > 0, what
        assert (z1 == -7.0).all() and (z2 == -7.0).all(), what          # a refused call writes nothing
    # more than 2^31 - 1 values S d: three empty segments of 2^30 components; refused before anything is allocated
    counts, sizes, ptrs, one = np.zeros(3, dtype=np.int64), np.ones(3, dtype=np.int32), (ctypes.c_void_p * 3)(), np.ones(3)
    assert lib.bluest_field_weighted_moments(3, 2 ** 30, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                             _lib.ptr(one), _lib.ptr(one), _lib.ptr(one), None) == ERR_ARG
    assert b"2^31" in lib.bluest_last_error()
    empty = np.ones((0, 3, 2))
    rc, zsum, zsq = raw([empty], np.ones(3))                            # no sample at all: zeros
    assert rc == 0 and (zsum == 0).all() and (zsq == 0).all()

"""
GPU tests of bluest_group_moments (include/bluest_hip.h Part 13, csrc/moments.hip) at its ABI: exact on small-integer data; the
bits of the numpy restatement of the documented order (tests/moments_ref.py) at every chunk edge, at every width at which the
launch takes another shape (csrc/moments.hip: L <= 4, 5..22, >= 23) and where the fold's lanes wrap; inside the rounding bound of a
long-double sum; independent of the other segments of the call, of host or device memory, of the alignment of the base and of
the slab size (the first-sample rows travel apart from the slabs); stable at a mean of 1e8; strict about its arguments.

Two kinds of data.  `general`: any float64, held to the restatement through the exact fma (Fraction), so only at shapes of at
most about 10^5 terms.  `moments_ref.data26`: values whose products are exact in float64, for which the restatement runs at numpy's
speed at any shape while the order of the additions still decides the bits.
"""
import ctypes

import numpy as np
import pytest

import gsums_ref
import moments_ref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

CHUNK = 128
COUNTS = (0, 1, 2, 15, 16, 17, 127, 128, 129, 8191, 8192, 8193)
WIDTHS = (1, 2, 3, 4, 5, 22, 23, 31, 32, 33, 40, 43, 63, 64)           # the issue's, both sides of the two shape breaks, and two
                                                                        # widths in between (the wide shape makes 2 .. 9 passes over the entries)
ERR_ARG = 1
U = gsums_ref.U
LD = np.longdouble


def general(n_out, N, L, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models"""
    rng = np.random.RandomState(seed)
    return 1.5 + 10.0 ** rng.uniform(-3, 3, L) * rng.randn(n_out, N, L)


def raw(segs, override=None):
    """the raw call on a list of host arrays / CUDA tensors [n_out, N, L]: (rc, first [n_out, T], second [n_out, P])"""
    from bluest_amd import _lib
    S = len(segs)
    n_out = int(segs[0].shape[0])
    counts = np.array([int(v.shape[1]) for v in segs], dtype=np.int64)
    sizes = np.array([int(v.shape[2]) for v in segs], dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(v) for v in segs])
    first = np.full((n_out, int(sizes.sum())), -7.0)
    second = np.full((n_out, int((sizes.astype(np.int64) * (sizes + 1) // 2).sum())), -7.0)
    args = dict(S=S, n_out=n_out, counts=_lib.ptr(counts), sizes=_lib.ptr(sizes), values=ctypes.cast(ptrs, ctypes.c_void_p),
                first=_lib.ptr(first), second=_lib.ptr(second), stream=None)
    for k, v in (override or {}).items():                              # an argument of the call replaced as it is
        args[k] = _lib.ptr(v) if isinstance(v, np.ndarray) else v
    rc = _lib.lib().bluest_group_moments(*[args[k] for k in ("S", "n_out", "counts", "sizes", "values", "first", "second", "stream")])
    return rc, first, second


def split(first, second, segs):
    out, c, p = [], 0, 0
    for v in segs:
        L = v.shape[2]
        out.append((first[:, c:c + L], second[:, p:p + L * (L + 1) // 2]))
        c, p = c + L, p + L * (L + 1) // 2
    return out


def same(got, want):
    return same_bits(got[0], want[0]) and same_bits(got[1], want[1])


@pytest.fixture(scope="module")
def pool():
    """42 ragged segments of data26 and the restatement's moments of each, computed once: counts around every chunk edge, zero and
    one sample in the middle, widths on both sides of every shape break, three outputs"""
    rng = np.random.RandomState(40)
    widths = list(WIDTHS) + rng.randint(1, 12, size=28).tolist()
    counts = [389, 5, 129, 0, 128, 17, 300, 1, 127, 16, 257, 200, 131, 130] + rng.randint(1, 300, size=28).tolist()
    segs = [moments_ref.data26(3, N, L, 2000 + i) for i, (N, L) in enumerate(zip(counts, widths))]
    return segs, [moments_ref.segment_moments(v, exact_products=True) for v in segs]


@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("L", WIDTHS)
def test_small_integers_are_summed_exactly(L, n_out):
    """integers below 8 in magnitude: every d is an integer below 16, every sum below 2^53, so any order gives the same answer"""
    rng = np.random.RandomState(L)
    segs = [rng.randint(-7, 8, size=(n_out, N, L)).astype(np.float64) for N in COUNTS]
    rc, first, second = raw(segs)
    assert rc == 0
    j, k = np.triu_indices(L)
    for v, (f, s) in zip(segs, split(first, second, segs)):
        d = v - v[:, :1, :] if v.shape[1] else v
        assert np.array_equal(f, d.sum(axis=1)), (L, n_out, v.shape[1])
        assert np.array_equal(s, (d[:, :, j] * d[:, :, k]).sum(axis=1)), (L, n_out, v.shape[1])
        if v.shape[1] < 2:                                              # no sample, or d = 0: +0.0 everywhere
            assert not np.signbit(f).any() and not np.signbit(s).any() and (f == 0).all() and (s == 0).all()


@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("L", WIDTHS)
def test_bits_of_the_restatement_at_every_chunk_edge(L, n_out):
    """data26 at every count (the three largest at the narrow widths here, at one width per launch shape in the next test), and
    general data through the exact fma at a few counts where the shape is small enough for it (at most 6e4 terms)"""
    P = L * (L + 1) // 2
    plain = [moments_ref.data26(n_out, N, L, 13 * L + N) for N in COUNTS if N <= 129 or L <= 5]
    slow = [general(n_out, N, L, 17 * L + N) for N in (2, 17, 129, 8193) if n_out * N * P <= 60000]
    assert slow
    rc, first, second = raw(plain + slow)
    assert rc == 0
    got = split(first, second, plain + slow)
    for i, v in enumerate(plain + slow):
        assert same(got[i], moments_ref.segment_moments(v, exact_products=i < len(plain))), (L, n_out, v.shape[1], i < len(plain))


@pytest.mark.parametrize("L", [3, 22, 64])
def test_more_chunks_than_fold_lanes(L):
    """64 and 65 chunks (8191, 8192, 8193 samples): the fold's lanes wrap; one width of every launch shape.  130 chunks at the two
    narrower ones: a lane takes a third chunk"""
    segs = [moments_ref.data26(1, N, L, L + N) for N in (8191, 8192, 8193)]
    if L < 64:
        segs.append(moments_ref.data26(1, 129 * CHUNK + 1, L, 5))
    rc, first, second = raw(segs)
    assert rc == 0
    for v, got in zip(segs, split(first, second, segs)):
        assert same(got, moments_ref.segment_moments(v, exact_products=True)), (L, v.shape[1])


def test_the_widest_segment_is_inside_the_long_double_bound():
    v = general(1, 8193, 64, 9)
    rc, first, second = raw([v])
    assert rc == 0
    s1, s2, a1, a2 = moments_ref.moments_ld(v)
    e1, e2 = np.abs(first.astype(LD) - s1), np.abs(second.astype(LD) - s2)
    b1, b2 = 2 * 8193 * U * a1, 2 * 8193 * U * a2
    print("largest error / bound: first", float((e1 / b1).max()), "second", float((e2 / b2).max()))
    assert (e1 <= b1).all() and (e2 <= b2).all()


def test_forty_two_segments_host_and_device_mixed(pool):
    import torch
    segs, want = pool
    mixed = [torch.from_numpy(v).cuda() if i % 3 == 1 and v.shape[1] > 0 else v for i, v in enumerate(segs)]
    torch.cuda.synchronize()
    rc, first, second = raw(mixed)
    assert rc == 0
    for i, (w, got) in enumerate(zip(want, split(first, second, segs))):
        assert same(got, w), (i, segs[i].shape)
    rc2, f2, s2 = raw(mixed)
    assert rc2 == 0 and same_bits(f2, first) and same_bits(s2, second)
    for v, got in zip(segs, split(first, second, segs)):                # and inside the rounding bound
        s1, sq, a1, a2 = moments_ref.moments_ld(v)
        N = v.shape[1]
        assert (np.abs(got[0].astype(LD) - s1) <= 2 * N * U * a1).all() and (np.abs(got[1].astype(LD) - sq) <= 2 * N * U * a2).all()


def test_a_segment_keeps_its_bits_alone_in_a_batch_on_the_device_and_at_another_base(pool):
    import torch
    segs, want = pool
    for i in (0, 4, 5, 6, 11, 12, 13):                                  # L = 1, 5, 22, 23, 43, 63, 64
        v = segs[i]
        rc, f, s = raw([v])
        assert rc == 0 and same((f, s), want[i])
        others = [segs[j] for j in (2, 8, 7)]
        for order in ([v] + others, others + [v], others[:2] + [v] + others[2:]):
            rc, f, s = raw(order)
            assert rc == 0 and same(split(f, s, order)[[k for k, o in enumerate(order) if o is v][0]], want[i])
        if v.shape[1] == 0:
            continue
        dev = torch.from_numpy(v).cuda()
        flat = torch.zeros(v.size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = torch.from_numpy(v).reshape(-1)
        shifted = flat[1:].reshape(v.shape)                             # 8- but not 16-byte aligned
        torch.cuda.synchronize()
        assert shifted.data_ptr() % 16 == 8 and dev.data_ptr() % 16 == 0
        for t in (dev, shifted):
            rc, f, s = raw([t])
            assert rc == 0 and same((f, s), want[i])
        host = np.zeros(v.size + 1)
        host[1:] = v.reshape(-1)
        rc, f, s = raw([host[1:].reshape(v.shape)])                     # the same from the host
        assert rc == 0 and same((f, s), want[i])


def test_a_tiny_slab_budget_gives_the_same_bits(pool):
    """the shift-row trap: under a budget of one chunk every later chunk of a host segment is staged without its first sample"""
    from bluest_amd import _lib, moments
    segs, want = pool
    big = [moments_ref.data26(2, 5 * CHUNK + 9, 7, 3), moments_ref.data26(2, 3, 4, 4), moments_ref.data26(2, 2 * CHUNK + 5, 30, 5)]
    ref = [moments_ref.segment_moments(v, exact_products=True) for v in big]
    rc, f, s = raw(big)
    assert rc == 0 and all(same(a, b) for a, b in zip(split(f, s, big), ref))
    lib, before = _lib.lib(), ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(1, ctypes.byref(before)) == 0 and before.value == 256 << 20
    try:
        rc1, f1, s1 = raw(big)                                          # room for one chunk of the widest segment: 6, 1 and 3 slabs
        assert lib.bluest_group_sums_slab(3 * CHUNK * 7 * 8 * 2 + 1000, None) == 0
        rc2, f2, s2 = raw(big)                                          # the first segment ends in the middle of a slab
        rc3, f3, s3 = raw(segs[:20])
    finally:
        assert lib.bluest_group_sums_slab(before.value, None) == 0
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    assert same_bits(f1, f) and same_bits(s1, s) and same_bits(f2, f) and same_bits(s2, s)
    assert all(same(a, b) for a, b in zip(split(f3, s3, segs[:20]), want[:20]))
    py = moments.group_moments(big, slab_bytes=1)                       # the Python entry sets the budget for its call only
    for (N, pf, ps), v, (rf, rs) in zip(py, big, ref):
        assert N == v.shape[1] and same_bits(pf, rf) and same_bits(ps, moments_ref.unpack(rs, v.shape[2]))
    now = ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(0, ctypes.byref(now)) == 0 and now.value == before.value


def test_a_mean_of_1e8_keeps_nine_digits_where_the_raw_sums_keep_none():
    """values = 1e8 + N(0, 1): the covariance from the shifted sums agrees with a two-pass long-double covariance to 1e-9 of
    sqrt(C_jj C_kk); sum y_j y_k - N ybar_j ybar_k in float64 on the same data does not"""
    from bluest_amd import moments
    rng = np.random.RandomState(8)
    A = np.eye(5) + 0.4
    v = 1e8 + rng.randn(2, 3000, 5) @ A.T
    C = moments.group_covariances([v])[0]
    want = moments_ref.covariance_ld(v)
    scale = np.sqrt(np.einsum("njj->nj", want))
    scale = scale[:, :, None] * scale[:, None, :]
    rel = (np.abs(C.astype(LD) - want) / scale).astype(np.float64)
    N = v.shape[1]
    raw_cov = (np.einsum("nij,nik->njk", v, v) - N * v.mean(axis=1)[:, :, None] * v.mean(axis=1)[:, None, :]) / (N - 1)
    rel_raw = (np.abs(raw_cov.astype(LD) - want) / scale).astype(np.float64)
    print("shifted sums:", rel.max(), "raw float64 sums:", rel_raw.max())
    assert rel.max() <= 1e-9
    assert rel_raw.max() > 1e-9


def test_nan_and_inf_propagate():
    v = general(1, 300, 3, 1)
    v[0, 200, 1] = np.nan
    w = general(1, 40, 2, 2)
    w[0, 7, 0] = np.inf
    x = general(1, 9, 2, 3)
    x[0, 0, 1] = np.inf                                                 # in the first sample: Inf - Inf = NaN in that column
    clean = general(1, 50, 3, 4)
    rc, first, second = raw([v, w, x, clean])
    assert rc == 0
    (fv, sv), (fw, sw), (fx, sx), (fc, sc) = split(first, second, [v, w, x, clean])
    assert np.isnan(fv[0, 1]) and np.isfinite(fv[0, [0, 2]]).all()
    assert np.isnan(sv[0, [1, 3, 4]]).all() and np.isfinite(sv[0, [0, 2, 5]]).all()    # pairs (0,1), (1,1), (1,2)
    assert np.isposinf(fw[0, 0]) and np.isfinite(fw[0, 1]) and np.isposinf(sw[0, 0]) and np.isinf(sw[0, 1]) and np.isfinite(sw[0, 2])
    assert np.isnan(fx[0, 1]) and np.isfinite(fx[0, 0]) and np.isnan(sx[0, [1, 2]]).all() and np.isfinite(sx[0, 0])
    assert same((fc, sc), moments_ref.segment_moments(clean))           # the neighbours are untouched


def test_argument_errors():
    from bluest_amd import _lib
    lib = _lib.lib()
    a, b = np.ones((1, 4, 3)), 2 * np.ones((1, 2, 2))
    a[0, 1:, 0] = [2, 3, 4]
    rc, first, second = raw([a, b])
    assert rc == 0 and first.tolist() == [[6.0, 0, 0, 0, 0]] and second.tolist() == [[14.0, 0, 0, 0, 0, 0, 0, 0, 0]]
    i64, i32 = (lambda *x: np.array(x, dtype=np.int64)), (lambda *x: np.array(x, dtype=np.int32))
    odd = np.zeros(4 * 3 * 8 + 8, dtype=np.uint8)[4:4 + 96]            # a base that is not 8-byte aligned
    bad = {"S = 0": dict(S=0), "S < 0": dict(S=-1), "n_out = 0": dict(n_out=0), "n_out = 1025": dict(n_out=1025),
           "counts": dict(counts=None), "sizes": dict(sizes=None), "values": dict(values=None), "first": dict(first=None),
           "second": dict(second=None), "size 0": dict(sizes=i32(3, 0)), "size 65": dict(sizes=i32(65, 2)),
           "negative count": dict(counts=i64(4, -1)),
           "null segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(_lib.ptr(a), None), ctypes.c_void_p)),
           "misaligned segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(odd.ctypes.data, _lib.ptr(b)), ctypes.c_void_p))}
    assert odd.ctypes.data % 8 == 4
    for what, change in bad.items():
        rc, f2, s2 = raw([a, b], override=change)
        assert rc == ERR_ARG, what
        assert len(lib.bluest_last_error()) > 0, what
        assert (f2 == -7.0).all() and (s2 == -7.0).all(), what          # a refused call writes nothing
    # more than 2^31 - 1 packed pairs: 1 032 445 empty segments of 64 models (2080 pairs each); refused before anything is allocated
    S = (2 ** 31 - 1) // 2080 + 1
    counts, sizes = np.zeros(S, dtype=np.int64), np.full(S, 64, dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)()
    one = np.zeros(1)
    call = lambda n: lib.bluest_group_moments(n, 1, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                              _lib.ptr(one), _lib.ptr(one), None)
    assert call(S) == ERR_ARG and b"pairs" in lib.bluest_last_error()
    empty = np.ones((1, 0, 3))
    rc, first, second = raw([empty])                                    # no sample at all: zeros
    assert rc == 0 and (first == 0).all() and (second == 0).all()

"""
GPU tests of bluest_field_group_moments (include/bluest_hip.h Part 16, csrc/field_cov.hip) at its ABI: exact on small integers;
the bits of the numpy restatement of the documented order (tests/field_cov_ref.py) at every chunk edge, at every (L, d) at which
the launch takes another shape and where the folds' lanes wrap; independent of the other segments of the call, of host or device
memory, of the alignment of the base, of the slab size and of whether `first` is asked for; anchored on the device to
bluest_group_moments and to bluest_field_weighted_moments; NaN and Inf stay in their segment.

Two kinds of data.  `general`: any float64, held to the restatement through the exact fma (Fraction), so only where
N L d <= 20000.  `field_moments_ref.data26` with weights that are powers of two or zero: the products are exact, so the
restatement runs at numpy's speed at any shape while the order of the additions still decides the bits.

The launch shape (csrc/field_cov.hip): a workgroup takes TB component tiles side by side, TB the largest power of two <= 16 with
n_pairs(L) TB <= 2304 and 8 L TB <= 2048 and below the number of tiles doubled; it stages sb samples at a time, sb the largest
power of two <= 16 with sb TB L 72 <= 40960 bytes.  `launch_shape` restates that rule.  With sixteen tiles and more, (TB, sb)
changes along L between 2 | 3, 4 | 5, 8 | 9, 16 | 17, 17 | 18, 23 | 24, 33 | 34, 35 | 36 and 47 | 48: EDGES holds both sides of each at
d = 128; a narrower d caps TB at 1, 2, 4 and 8 (d = 8, 9, 25, 64 among the shapes; (9, 17) is the one place where TB = 4 meets sb = 8).
"""
import ctypes

import numpy as np
import pytest

import field_cov_ref as ref
import field_moments_ref
import gsums_ref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

CHUNK = 128
COUNTS = (0, 1, 2, 15, 16, 17, 127, 128, 129, 8191, 8192, 8193)
LS = (1, 2, 3, 5, 32, 64)
DS = (1, 2, 7, 8, 9, 63, 64, 65, 257)
BREAKS = [(2, 3), (4, 5), (8, 9), (16, 17), (17, 18), (23, 24), (33, 34), (35, 36), (47, 48)]
EDGES = sorted(set((L, 128) for pair in BREAKS for L in pair)) + [(3, 25), (9, 17)]
SHAPES = sorted(set((L, d) for L in LS for d in DS) | set(EDGES))
ERR_ARG = 1


def launch_shape(L, d):
    """(tiles per workgroup, samples per sub-block)"""
    ntiles, npairs = (d + 7) // 8, L * (L + 1) // 2
    tb = 1
    while tb < 16 and tb < ntiles and npairs * 2 * tb <= 9 * 256 and L * 8 * 2 * tb <= 8 * 256:
        tb *= 2
    sb = 16
    while sb > 1 and sb * tb * L * 9 * 8 > 40 * 1024:
        sb //= 2
    return tb, sb


def counts_for(L, d):
    """the large counts only where L d <= 320"""
    return [N for N in COUNTS if N <= 129 or L * d <= 320]


def general(N, L, d, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models"""
    rng = np.random.RandomState(seed)
    return 1.5 + 10.0 ** rng.uniform(-3, 3, L)[None, :, None] * rng.randn(N, L, d)


def exact(N, L, d, seed):
    return field_moments_ref.data26(N, L, d, seed)[0]


def raw(segs, w, with_first=True):
    """the raw call on a list of host arrays / CUDA tensors [N, L, d]: (rc, per segment (second [P_s], cross [P_s], first [L_s, d]))"""
    from bluest_amd import _lib
    S, d = len(segs), int(segs[0].shape[2])
    counts = np.array([int(v.shape[0]) for v in segs], dtype=np.int64)
    sizes = np.array([int(v.shape[1]) for v in segs], dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(v) if v.shape[0] > 0 else None for v in segs])
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    assert w.shape == (d,)
    tri = sizes.astype(np.int64) * (sizes + 1) // 2
    second, cross = np.full(int(tri.sum()), -7.0), np.full(int(tri.sum()), -7.0)
    first = np.full((int(sizes.sum()), d), -7.0) if with_first else None
    rc = _lib.lib().bluest_field_group_moments(S, d, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p), _lib.ptr(w),
                                               _lib.ptr(second), _lib.ptr(cross), _lib.ptr(first), None)
    p0, c0 = np.cumsum(tri) - tri, np.cumsum(sizes) - sizes
    return rc, [(second[p0[s]:p0[s] + tri[s]], cross[p0[s]:p0[s] + tri[s]], None if first is None else first[c0[s]:c0[s] + sizes[s]])
                for s in range(S)]


def same(got, want):
    """(second, cross, first) against the restatement's (first, second, cross)"""
    return same_bits(got[0], want[1]) and same_bits(got[1], want[2]) and (got[2] is None or same_bits(got[2], want[0]))


def test_the_shapes_cover_every_launch_shape():
    everywhere = {launch_shape(L, d) for L in range(1, 65) for d in range(1, 300)}
    assert {launch_shape(L, d) for L, d in SHAPES} == everywhere
    assert {tb for tb, _ in everywhere} == {1, 2, 4, 8, 16} and {sb for _, sb in everywhere} == {2, 4, 8, 16}
    at128 = [launch_shape(L, 128) for L in range(1, 65)]
    assert [(L, L + 1) for L in range(1, 64) if at128[L - 1] != at128[L]] == BREAKS        # every break along L, both sides among EDGES
    assert all((L, 128) in SHAPES for pair in BREAKS for L in pair)
    assert [launch_shape(3, d)[0] for d in (8, 9, 16, 17, 32, 33, 64, 65)] == [1, 2, 2, 4, 4, 8, 8, 16]   # the cap by the tiles there are
    assert launch_shape(64, 257) == (1, 8) and launch_shape(1, 257) == (16, 16) and launch_shape(16, 128) == (16, 2)


@pytest.mark.parametrize("L,d", SHAPES)
def test_small_integers_are_summed_exactly(L, d):
    """values below 8 in magnitude and integer weights below 4: every sum is an integer below 2^53, so any order gives it"""
    rng = np.random.RandomState(100 * L + d)
    segs = [rng.randint(-7, 8, size=(N, L, d)).astype(np.float64) for N in counts_for(L, d)]
    w = rng.randint(0, 4, size=d).astype(np.float64)
    rc, got = raw(segs, w)
    assert rc == 0
    j, k = np.triu_indices(L)
    for v, (second, cross, first) in zip(segs, got):
        dv = v - v[:1] if v.shape[0] else v
        f = dv.sum(axis=0)
        assert np.array_equal(first, f), (L, d, v.shape[0])
        assert np.array_equal(second, np.einsum("ipc,c,ipc->p", dv[:, j], w, dv[:, k])), (L, d, v.shape[0])
        assert np.array_equal(cross, np.einsum("pc,c,pc->p", f[j], w, f[k])), (L, d, v.shape[0])
        if v.shape[0] < 2:                                              # no sample, or d = 0: +0.0 everywhere
            assert not any(np.signbit(a).any() or a.any() for a in (second, cross, first))


@pytest.mark.parametrize("L,d", SHAPES)
def test_bits_of_the_restatement_at_every_chunk_edge(L, d):
    """exact-chain data at every count in one call, and general data through the exact fma where N L d <= 20000"""
    w = ref.weights_pow2(d, L + d)
    plain = [exact(N, L, d, 13 * L + 7 * d + N) for N in counts_for(L, d)]
    rc, got = raw(plain, w)
    assert rc == 0
    for v, g in zip(plain, got):
        assert same(g, ref.segment_moments(v, w, exact_products=True)), (L, d, v.shape[0])
    slow = [general(N, L, d, 17 * L + N) for N in (2, 17, 129) if N * L * d <= 20000]
    if slow:
        wg = np.random.RandomState(d).uniform(0.0, 3.0, d)
        rc, got = raw(slow, wg)
        assert rc == 0
        for v, g in zip(slow, got):
            assert same(g, ref.segment_moments(v, wg)), (L, d, v.shape[0])


@pytest.mark.parametrize("L,d", [(1, 513), (3, 513), (1, 1025), (3, 1025)])
def test_more_tiles_than_fold_lanes(L, d):
    """65 tiles: the lanes of the tile fold wrap; 129 tiles: a lane takes a third tile"""
    w = ref.weights_pow2(d, d)
    segs = [exact(N, L, d, L + d + N) for N in (2, 17, 129)]
    rc, got = raw(segs, w)
    assert rc == 0
    for v, g in zip(segs, got):
        assert same(g, ref.segment_moments(v, w, exact_products=True)), (L, d, v.shape[0])


@pytest.fixture(scope="module", params=[3, 70])
def pool(request):
    """24 ragged segments of exact-chain data with d = 3 or d = 70 and the restatement's results, computed once: counts around
    every chunk edge, zero and one sample in the middle, group sizes on either side of the launch-shape breaks"""
    d = request.param
    rng = np.random.RandomState(40 + d)
    sizes = [1, 2, 3, 5, 9, 16, 17, 24, 33, 36, 48, 64] + rng.randint(1, 12, size=12).tolist()
    counts = [389, 5, 129, 0, 128, 17, 300, 1, 127, 16, 257, 131] + rng.randint(1, 300, size=12).tolist()
    w = ref.weights_pow2(d, d)
    segs = [exact(N, L, d, 3000 + i) for i, (N, L) in enumerate(zip(counts, sizes))]
    return segs, w, [ref.segment_moments(v, w, exact_products=True) for v in segs]


def test_ragged_segments_host_and_device_mixed(pool):
    import torch
    segs, w, want = pool
    mixed = [torch.from_numpy(v).cuda() if i % 3 == 1 and v.shape[0] > 0 else v for i, v in enumerate(segs)]
    torch.cuda.synchronize()
    rc, got = raw(mixed, w)
    assert rc == 0
    for i, (g, wnt) in enumerate(zip(got, want)):
        assert same(g, wnt), (i, segs[i].shape)
    rc, again = raw(mixed, w, with_first=False)                         # `first` null: second and cross keep their bits
    assert rc == 0 and all(a[2] is None and same_bits(a[0], g[0]) and same_bits(a[1], g[1]) for a, g in zip(again, got))


def test_a_segment_keeps_its_bits_alone_in_a_batch_on_the_device_and_at_another_base(pool):
    import torch
    segs, w, want = pool
    for i in (0, 2, 4, 6, 8, 10, 11):                                   # L = 1, 3, 9, 17, 33, 48, 64
        v = segs[i]
        rc, got = raw([v], w)
        assert rc == 0 and same(got[0], want[i])
        others = [1, 9, 5]
        for order in ([i] + others, others + [i], others[:2] + [i] + others[2:]):
            rc, got = raw([segs[k] for k in order], w)
            assert rc == 0 and same(got[order.index(i)], want[i])
        dev = torch.from_numpy(v).cuda()
        flat = torch.zeros(v.size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = torch.from_numpy(v).reshape(-1)
        shifted = flat[1:].reshape(v.shape)                             # 8- but not 16-byte aligned
        torch.cuda.synchronize()
        assert shifted.data_ptr() % 16 == 8 and dev.data_ptr() % 16 == 0
        host = np.zeros(v.size + 1)
        host[1:] = v.reshape(-1)
        for t in (dev, shifted, host[1:].reshape(v.shape)):
            rc, got = raw([t], w)
            assert rc == 0 and same(got[0], want[i])


def test_every_slab_budget_gives_the_same_bits(pool):
    """the shift-row trap: under a budget of one chunk every later chunk of a host segment is staged without its first sample"""
    from bluest_amd import _lib, field_covariances
    segs, w, want = pool
    d = segs[0].shape[2]
    big = [exact(5 * CHUNK + 9, 7, d, 3), exact(3, 4, d, 4), exact(2 * CHUNK + 5, 30, d, 5)]
    want_big = [ref.segment_moments(v, w, exact_products=True) for v in big]
    rc, got = raw(big, w)
    assert rc == 0 and all(same(g, wnt) for g, wnt in zip(got, want_big))
    lib, before = _lib.lib(), ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(1, ctypes.byref(before)) == 0 and before.value == 256 << 20
    try:
        rc1, got1 = raw(big, w)                                         # room for one chunk of the widest segment
        assert lib.bluest_group_sums_slab(3 * CHUNK * 7 * d * 8 + 1000, None) == 0
        rc2, got2 = raw(big, w)                                         # the first segment ends in the middle of a slab
        assert lib.bluest_group_sums_slab(1 << 20, None) == 0
        rc3, got3 = raw(segs, w)
    finally:
        assert lib.bluest_group_sums_slab(before.value, None) == 0
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    assert all(same(g, wnt) for g, wnt in zip(got1, want_big)) and all(same(g, wnt) for g, wnt in zip(got2, want_big))
    assert all(same(g, wnt) for g, wnt in zip(got3, want))
    py = field_covariances.field_group_moments(big, w, with_first=True, slab_bytes=1)      # the Python entry sets the budget for its call only
    for (N, second, cross, first), v, wnt in zip(py, big, want_big):
        L = v.shape[1]
        assert N == v.shape[0] and same_bits(second, ref.unpack(wnt[1], L)) and same_bits(cross, ref.unpack(wnt[2], L)) and same_bits(first, wnt[0])
    now = ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(0, ctypes.byref(now)) == 0 and now.value == before.value


@pytest.mark.parametrize("L", [1, 3, 22, 23, 64])
def test_at_one_component_it_is_group_moments_on_the_device(L):
    """d = 1 and w = 1: `second` and `first` are bit for bit those of bluest_group_moments (n_out = 1) on the same values"""
    from bluest_amd import moments
    segs = [general(N, L, 1, 5 * N + L) for N in (1, 2, 17, 129, 1000)]
    rc, got = raw(segs, [1.0])
    assert rc == 0
    j, k = np.triu_indices(L)
    for (N, first, second), (g2, gx, g1) in zip(moments.group_moments([np.ascontiguousarray(v[None, :, :, 0]) for v in segs]), got):
        assert same_bits(g1[:, 0], first[0]) and same_bits(g2, second[0][j, k]), (L, N)
        assert same_bits(gx, first[0][j] * first[0][k])


@pytest.mark.parametrize("d", [1, 9])
def test_one_model_and_a_one_hot_weight_are_the_weighted_moments_on_the_device(d):
    """sizes 1 and w one-hot at c: `second` is bit for bit zsq[s][c] of bluest_field_weighted_moments with coefficient 1.0, and
    `first` its zsum"""
    from bluest_amd import field_errors
    segs = [general(N, 1, d, 3 * N + d) for N in (1, 2, 17, 129, 1000)]
    moms = field_errors.field_weighted_moments(segs, np.ones(len(segs)))
    for c in range(d):
        w = np.zeros(d)
        w[c] = 1.0
        rc, got = raw(segs, w)
        assert rc == 0
        for (N, zsum, zsq), (second, cross, first) in zip(moms, got):
            assert same_bits(second, zsq[c:c + 1]) and same_bits(first[0], zsum), (d, c, N)
            assert same_bits(cross, zsum[c:c + 1] ** 2)


@pytest.mark.parametrize("d", [3, 65])
def test_nan_and_inf_propagate_and_stay_in_their_segment(d):
    v = general(300, 3, d, 1)
    v[200, 1, 2] = np.nan
    x = general(40, 2, d, 2)
    x[7, 0, 1] = np.inf
    y = general(9, 2, d, 3)
    y[0, 1, 0] = np.inf                                                 # in the first sample: Inf - Inf = NaN
    clean = general(50, 3, d, 4)
    w = np.random.RandomState(d).uniform(0.5, 2.0, d)
    rc, got = raw([v, x, y, clean], w)
    assert rc == 0
    j3, k3 = np.triu_indices(3)
    touched = (j3 == 1) | (k3 == 1)
    assert np.isnan(got[0][0][touched]).all() and np.isfinite(got[0][0][~touched]).all()
    assert np.isnan(got[0][1][touched]).all() and np.isfinite(got[0][1][~touched]).all() and np.isnan(got[0][2][1, 2])
    assert np.isposinf(got[1][0][0]) and np.isposinf(got[1][2][0, 1]) and np.isfinite(got[1][0][2])
    assert np.isnan(got[2][0][2]) and np.isnan(got[2][2][1, 0]) and np.isfinite(got[2][0][0])
    assert same(got[3], ref.segment_moments(clean, w))                  # the neighbours are untouched

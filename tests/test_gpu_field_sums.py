"""
GPU tests of bluest_field_sums (include/bluest_hip.h Part 12, csrc/fields.hip) at its ABI: the bits of bluest_group_sums at d = 1,
the bits of the numpy restatement (tests/fields_ref.py: steps 1-3 of Part 11 per column and component) over every chunk edge,
width and component count, independent of the other segments, of host or device memory and of the slab size, mu in the stated
fma order, and strict about its arguments.
"""
import ctypes

import numpy as np
import pytest

import fields_ref
from fields_ref import same_bits

pytestmark = pytest.mark.gpu

CHUNK = 128
COUNTS = (0, 1, 16, 17, 128, 129, 64 * 128 + 1)
ERR_ARG = 1


def data(N, L, d, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the columns and components: sums whose bits depend on the order"""
    rng = np.random.RandomState(seed)
    return 1.5 + 10.0 ** rng.uniform(-3, 3, (L, d)) * rng.randn(N, L, d)


def raw(segs, weights=None, repeat_of=None, R=0, override=None):
    """the raw call on a list of host arrays / CUDA tensors [N, L, d]: (rc, sums [T, d], mu [R, d] or None)"""
    from bluest_amd import _lib
    S, d = len(segs), int(segs[0].shape[2])
    assert all(int(v.shape[2]) == d for v in segs), "one call takes one component count"
    counts = np.array([int(v.shape[0]) for v in segs], dtype=np.int64)
    sizes = np.array([int(v.shape[1]) for v in segs], dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(v) for v in segs])
    T = int(sizes.sum())
    sums = np.full((T, d), -7.0)
    weights = None if weights is None else np.ascontiguousarray(weights, dtype=np.float64)
    mu = None if weights is None else np.full((R, d), -7.0)
    rep = None if repeat_of is None else np.asarray(repeat_of, dtype=np.int64)
    args = dict(S=S, d=d, counts=_lib.ptr(counts), sizes=_lib.ptr(sizes), values=ctypes.cast(ptrs, ctypes.c_void_p),
                weights=_lib.ptr(weights), R=R, repeat_of=_lib.ptr(rep), sums=_lib.ptr(sums), mu=_lib.ptr(mu), stream=None)
    for k, v in (override or {}).items():                              # an argument of the call replaced as it is
        args[k] = _lib.ptr(v) if isinstance(v, np.ndarray) else v
    rc = _lib.lib().bluest_field_sums(*[args[k] for k in ("S", "d", "counts", "sizes", "values", "weights", "R", "repeat_of", "sums",
                                                          "mu", "stream")])
    return rc, sums, mu


def split(sums, segs):
    out, c = [], 0
    for v in segs:
        out.append(sums[c:c + v.shape[1]])
        c += v.shape[1]
    return out


@pytest.fixture(scope="module")
def pool():
    """the ragged segments of every count, a few widths and component counts, and the restatement's sums of each, computed once"""
    segs = {}
    for d in (1, 5, 257):
        for L in (1, 3, 64):
            counts = COUNTS if L * d <= 320 else COUNTS[:-1] + (2 * CHUNK + 1,)      # the 65-chunk segment where it stays small
            segs[d, L] = [data(N, L, d, 1000 * d + 10 * L + i) for i, N in enumerate(counts)]
    return segs, {k: [fields_ref.segment_sums(v) for v in vs] for k, vs in segs.items()}


def test_one_component_has_the_bits_of_the_group_sums(pool):
    from bluest_amd import _lib
    segs = [v for L in (1, 3, 64) for v in pool[0][1, L]]
    rc, sums, _ = raw(segs)
    S = len(segs)
    flat = [np.ascontiguousarray(v[None, :, :, 0]) for v in segs]       # [1, N, L]
    counts = np.array([v.shape[1] for v in flat], dtype=np.int64)
    sizes = np.array([v.shape[2] for v in flat], dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(v) for v in flat])
    want = np.full((1, int(sizes.sum())), -7.0)
    assert _lib.lib().bluest_group_sums(S, 1, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p), None, 0, None,
                                        _lib.ptr(want), None, None) == 0
    assert rc == 0 and same_bits(sums[:, 0], want[0])


@pytest.mark.parametrize("d", [1, 5, 257])
def test_bits_of_the_restatement_for_ragged_segments(d, pool):
    segs = [v for (dd, L), vs in pool[0].items() if dd == d for v in vs]
    want = [w for (dd, L), ws in pool[1].items() if dd == d for w in ws]
    rc, sums, _ = raw(segs)
    assert rc == 0
    for v, got, w in zip(segs, split(sums, segs), want):
        assert same_bits(got, w), (d, v.shape)
        if v.shape[0] == 0:
            assert not got.any() and not np.signbit(got).any()


def test_a_segment_keeps_its_bits_alone_in_a_batch_on_the_device_and_under_a_tiny_slab(pool):
    import torch
    from bluest_amd import _lib, fields
    segs, want = pool
    others = [segs[5, 1][3], segs[5, 64][5]]
    for key, i in (((5, 3), 5), ((5, 64), 4), ((5, 1), 6), ((5, 3), 2)):
        v, w = segs[key][i], want[key][i]
        rc, alone, _ = raw([v])
        assert rc == 0 and same_bits(alone, w)
        for order in ([v] + others, others + [v], others[:1] + [v] + others[1:]):
            rc, sums, _ = raw(order)
            assert rc == 0 and same_bits(split(sums, order)[[k for k, o in enumerate(order) if o is v][0]], w)
        T = torch.from_numpy(v).cuda()
        torch.cuda.synchronize()
        rc, dev, _ = raw([T])
        assert rc == 0 and same_bits(dev, w)
        rc, mixed, _ = raw([others[0], T, others[1]])
        assert rc == 0 and same_bits(split(mixed, [others[0], v, others[1]])[1], w)
    batch = segs[5, 3] + segs[5, 64]
    lib, before = _lib.lib(), ctypes.c_int64(0)
    rc, whole, _ = raw(batch)
    assert rc == 0 and lib.bluest_group_sums_slab(1, ctypes.byref(before)) == 0
    try:
        rc1, tiny, _ = raw(batch)                                       # room for one chunk of the widest segment
    finally:
        assert lib.bluest_group_sums_slab(before.value, None) == 0
    assert rc1 == 0 and same_bits(tiny, whole)
    py = fields.field_group_sums(batch, slab_bytes=1)
    assert all(same_bits(a, b) for a, b in zip(py, want[5, 3] + want[5, 64]))


def test_mu_in_the_stated_fma_order_with_a_repeat_without_segments(pool):
    from bluest_amd import fields
    segs, want = pool
    pick = [segs[5, 3][4], segs[5, 1][0], segs[5, 64][3], segs[5, 3][6], segs[5, 1][2]]         # a zero count among them
    T = sum(v.shape[1] for v in pick)
    W = np.random.RandomState(3).randn(T) * 10.0 ** np.random.RandomState(4).uniform(-2, 2, T)
    for repeat_of, R in (([0] * 5, 1), ([0, 0, 1, 3, 3], 4), ([0, 1, 1, 1, 2], 5)):
        rc, sums, mu = raw(pick, weights=W, repeat_of=repeat_of, R=R)
        ref_sums, ref_mu = fields_ref.field_group_sums(pick, W, repeat_of, R)
        assert rc == 0 and same_bits(sums, np.concatenate(ref_sums, axis=0)) and same_bits(mu, ref_mu), repeat_of
    assert not mu[3:].any() and mu[:3].all()
    rc, sums, mu = raw(pick, weights=W, repeat_of=[0, 0, 1, 3, 3], R=4)
    assert rc == 0 and not mu[2].any() and not np.signbit(mu[2]).any()  # a repeat without segments
    out, py = fields.field_group_sums(pick, weights=W, repeat_of=[0, 0, 1, 3, 3])
    assert same_bits(py, mu) and all(same_bits(a, b) for a, b in zip(out, ref_sums))


def test_sums_are_inside_the_rounding_bound(pool):
    segs, _ = pool
    for batch in (segs[257, 3] + segs[257, 1], segs[5, 64] + segs[5, 3]):         # one component count per call
        rc, sums, _ = raw(batch)
        assert rc == 0
        for v, got in zip(batch, split(sums, batch)):
            exact, absolute = fields_ref.segment_ld(v)
            bound = (2 * v.shape[0] * fields_ref.U * absolute).astype(np.float64)
            assert (np.abs(got.astype(fields_ref.LD) - exact).astype(np.float64) <= bound).all()


def test_argument_errors():
    from bluest_amd import _lib
    lib = _lib.lib()
    a, b = np.ones((4, 3, 2)), 2 * np.ones((2, 2, 2))
    W = np.ones(5)
    rc, sums, mu = raw([a, b], weights=W, repeat_of=[0, 1], R=2)
    assert rc == 0 and sums.tolist() == [[4.0, 4.0]] * 5 and mu.tolist() == [[12.0, 12.0], [8.0, 8.0]]
    i64, i32 = (lambda *x: np.array(x, dtype=np.int64)), (lambda *x: np.array(x, dtype=np.int32))
    bad = {"S = 0": dict(S=0), "S < 0": dict(S=-1), "d = 0": dict(d=0), "d < 0": dict(d=-1),
           "counts": dict(counts=None), "sizes": dict(sizes=None), "values": dict(values=None), "sums": dict(sums=None),
           "size 0": dict(sizes=i32(3, 0)), "size 65": dict(sizes=i32(65, 2)), "negative count": dict(counts=i64(4, -1)),
           "decreasing repeat_of": dict(repeat_of=i64(1, 0)), "repeat_of out of range": dict(repeat_of=i64(0, 2)),
           "repeat_of < 0": dict(repeat_of=i64(-1, 0)), "weights without mu": dict(mu=None), "mu without weights": dict(weights=None),
           "weights without repeat_of": dict(repeat_of=None), "R = 0": dict(R=0), "too many column-components": dict(d=1 << 29),
           "null segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(_lib.ptr(a), None), ctypes.c_void_p)),
           "misaligned segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(_lib.ptr(a) + 4, _lib.ptr(b)), ctypes.c_void_p))}
    for what, change in bad.items():
        rc, s2, m2 = raw([a, b], weights=W, repeat_of=[0, 1], R=2, override=change)
        assert rc == ERR_ARG, what
        assert len(lib.bluest_last_error()) > 0, what
        assert (s2 == -7.0).all() and (m2 is None or (m2 == -7.0).all()), what          # a refused call writes nothing
    rc, sums, _ = raw([np.ones((0, 3, 2))])                             # no sample at all: zeros
    assert rc == 0 and not sums.any()

"""GPU tests of bluest_field_pilot_moments (include/bluest_hip.h, Part 17; csrc/field_pilot.hip) at its ABI: bit for bit against
the numpy restatement tests/field_pilot_ref.py at the smallest shapes that reach every launch shape (one sample per workgroup at
wide L, many at narrow L, column blocks narrower than 64 where d < 64 or L is wide), every edge of column block, strip and chunk,
and one or several strips; the same bits from host and device memory, at a base offset by 8 bytes, under a staging budget and a
scratch limit of one chunk; the anchors the header states; and every BLUEST_ERR_ARG case."""
import functools

import numpy as np
import pytest

import field_pilot_ref as ref
from field_pilot_ref import same_bits

pytestmark = pytest.mark.gpu

# (N, L, d): N over {1, 2, 127, 128, 129, 300} (chunk of 128), L over {1, 2, 3, 8, 17, 33, 64}, d over {1, 7, 8, 9, 63, 64, 65, 511,
# 512, 513, 1100} (column blocks of at most 64, strips of 512).  The restatement costs N L (L + 1) d exact fmas, so the large values
# of the three meet only in pairs.
CASES = list(dict.fromkeys(
    [(N, 1, 1) for N in (1, 2, 127, 128, 129, 300)] +
    [(N, 3, 9) for N in (1, 2, 127, 128, 129, 300)] +
    [(N, 2, 65) for N in (127, 128, 129, 300)] +
    [(3, L, 9) for L in (1, 2, 3, 8, 17, 33, 64)] +
    [(2, L, 1) for L in (2, 8, 17, 33, 64)] +
    [(2, 3, d) for d in (1, 7, 8, 9, 63, 64, 65, 511, 512, 513, 1100)] +
    [(129, 8, 7), (128, 17, 8), (129, 8, 65), (40, 17, 63), (2, 64, 64), (2, 64, 65), (1, 33, 65), (2, 33, 513), (1, 64, 513),
     (3, 8, 1100), (2, 17, 1100), (130, 3, 513), (129, 2, 1100), (300, 2, 513), (127, 3, 511), (128, 1, 512), (300, 1, 64),
     (300, 2, 8), (260, 8, 9), (300, 1, 7)]
))


@functools.lru_cache(maxsize=None)
def data(N, L, d):
    """mean 1.5, scales from 1e-2 to 1e2 across the models, models 0 and 1 close together; weights in (0, 2); the centre is the
    float64 mean"""
    rng = np.random.RandomState(1000 * N + 10 * L + d)
    scale = 10.0 ** rng.uniform(-2, 2, (L, 1))
    Y = 1.5 + scale * rng.randn(N, L, d)
    if L > 1:
        Y[:, 1] = Y[:, 0] + 1e-6 * rng.randn(N, d)
    w = rng.uniform(0.0, 2.0, d)
    return Y, w, Y.mean(axis=0)


@functools.lru_cache(maxsize=None)
def expected(N, L, d):
    return ref.pilot_moments(*data(N, L, d))


def call(values, w, centre, **kw):
    from bluest_amd.field_pilot_errors import field_pilot_moments
    return field_pilot_moments(values, w, centre, **kw)


def all_same(xs, ys):
    return all((a is None and b is None) or (a is not None and b is not None and same_bits(a, b)) for a, b in zip(xs, ys))


@pytest.mark.parametrize("N,L,d", CASES)
def test_the_bits_of_the_restatement(N, L, d):
    got, want = call(*data(N, L, d)), expected(N, L, d)
    for name, a, b in zip(("qfirst", "qs1", "qs2", "rfirst", "rs1", "rs2"), got, want):
        assert same_bits(a, b), (name, np.abs(a - b).max())
    assert np.array_equal(got[0], got[0].T) and np.array_equal(got[1], got[1].T) and np.array_equal(got[2], got[2].T)
    assert not np.tril(got[3]).any() and not np.tril(got[4]).any() and not np.tril(got[5]).any()


SHAPES = [(300, 3, 9), (300, 2, 513), (260, 8, 9), (129, 2, 1100)]


@pytest.mark.parametrize("N,L,d", SHAPES)
def test_the_same_bits_from_host_and_device_memory_at_any_alignment(N, L, d):
    import torch
    Y, w, centre = data(N, L, d)
    want = expected(N, L, d)
    dev = torch.from_numpy(Y).cuda()
    assert all_same(call(dev, w, centre), want)
    flat = torch.empty(Y.size + 1, dtype=torch.float64, device="cuda")
    shifted = flat[1:].view(N, L, d)
    shifted.copy_(dev)
    assert shifted.data_ptr() % 16 == 8 or dev.data_ptr() % 16 == 8
    assert all_same(call(shifted, w, centre), want)
    host = np.empty(Y.size + 1)
    moved = host[1:].reshape(N, L, d)
    moved[...] = Y
    assert moved.ctypes.data % 16 != Y.ctypes.data % 16
    assert all_same(call(moved, w, centre), want)


@pytest.mark.parametrize("N,L,d", SHAPES)
def test_the_same_bits_under_any_staging_budget_and_scratch_limit(N, L, d):
    import torch
    Y, w, centre = data(N, L, d)
    want = expected(N, L, d)
    assert all_same(call(Y, w, centre, slab_bytes=1), want)             # host input, one chunk per slab
    assert all_same(call(Y, w, centre, scratch_bytes=1), want)          # one chunk per run
    assert all_same(call(torch.from_numpy(Y).cuda(), w, centre, scratch_bytes=1), want)
    assert all_same(call(Y, w, centre, slab_bytes=2 * 128 * L * d * 8, scratch_bytes=1 << 40), want)


def test_zero_weights_drop_their_components():
    Y, w, centre = data(129, 8, 65)
    keep = np.ones(65, dtype=bool)
    keep[[0, 7, 8, 31, 64]] = False
    w0 = np.where(keep, w, 0.0)
    assert all_same(call(Y, w0, centre), call(np.ascontiguousarray(Y[:, :, keep]), w[keep], np.ascontiguousarray(centre[:, keep])))


@pytest.mark.parametrize("k", [0, 4, 8])
def test_a_one_hot_weight_is_the_call_on_that_component(k):
    Y, w, centre = data(300, 3, 9)
    e = np.zeros(9)
    e[k] = 1.0
    assert all_same(call(Y, e, centre), call(np.ascontiguousarray(Y[:, :, k:k + 1]), np.ones(1), np.ascontiguousarray(centre[:, k:k + 1])))


@pytest.mark.parametrize("s", [0, 200])
def test_one_nan_reaches_exactly_the_pairs_of_its_model(s):
    Y, w, centre = data(300, 3, 9)
    Y = Y.copy()
    Y[s, 1, 4] = np.nan
    got, clean = call(Y, w, centre), expected(300, 3, 9)
    hit = np.zeros((3, 3), dtype=bool)
    hit[1, :] = hit[:, 1] = True
    upper = np.triu(np.ones((3, 3), dtype=bool), 1)
    for k, (a, b) in enumerate(zip(got, clean)):
        touched = hit if k < 3 else hit & upper
        sums = k % 3 != 0 or s == 0                                     # the first sample's value sees only a NaN of sample 0
        assert np.isnan(a[touched]).all() == sums and (sums or same_bits(a, b))
        assert same_bits(a[~touched], b[~touched])


def test_without_the_difference_outputs_the_q_bits_stay():
    for shape in [(300, 3, 9), (2, 64, 65), (129, 2, 1100)]:
        got = call(*data(*shape), differences=False)
        assert got[3] is None and got[4] is None and got[5] is None
        assert all_same(got[:3], expected(*shape)[:3])


def raw(N, L, d, values, w, centre, outs):
    from bluest_amd import _lib
    return _lib.lib().bluest_field_pilot_moments(N, L, d, _lib.ptr(values), _lib.ptr(w), _lib.ptr(centre), *[_lib.ptr(a) for a in outs], None)


def test_argument_errors_launch_nothing():
    from bluest_amd import _lib
    Y, w, centre = data(3, 3, 9)
    fresh = lambda: [np.full((3, 3), -7.0) for _ in range(6)]
    bad_w, inf_w, nan_w = w.copy(), w.copy(), w.copy()
    bad_w[2], inf_w[3], nan_w[8] = -1.0, np.inf, np.nan
    odd = np.frombuffer(np.zeros(Y.nbytes + 8, dtype=np.uint8).data, dtype=np.float64, count=Y.size, offset=4)
    assert odd.ctypes.data % 8 == 4
    cases = {
        "values not 8-byte aligned": lambda o: raw(3, 3, 9, odd, w, centre, o),
        "L = 0": lambda o: raw(3, 0, 9, Y, w, centre, o),
        "L = 65": lambda o: raw(3, 65, 9, Y, w, centre, o),
        "d = 0": lambda o: raw(3, 3, 0, Y, w, centre, o),
        "N = 0": lambda o: raw(0, 3, 9, Y, w, centre, o),
        "null values": lambda o: raw(3, 3, 9, None, w, centre, o),
        "null w": lambda o: raw(3, 3, 9, Y, None, centre, o),
        "null centre": lambda o: raw(3, 3, 9, Y, w, None, o),
        "null qfirst": lambda o: raw(3, 3, 9, Y, w, centre, [None] + o[1:]),
        "null qs1": lambda o: raw(3, 3, 9, Y, w, centre, o[:1] + [None] + o[2:]),
        "null qs2": lambda o: raw(3, 3, 9, Y, w, centre, o[:2] + [None] + o[3:]),
        "only rfirst null": lambda o: raw(3, 3, 9, Y, w, centre, o[:3] + [None] + o[4:]),
        "only rs1 null": lambda o: raw(3, 3, 9, Y, w, centre, o[:4] + [None] + o[5:]),
        "only rs2 given": lambda o: raw(3, 3, 9, Y, w, centre, o[:3] + [None, None] + o[5:]),
        "negative weight": lambda o: raw(3, 3, 9, Y, bad_w, centre, o),
        "infinite weight": lambda o: raw(3, 3, 9, Y, inf_w, centre, o),
        "NaN weight": lambda o: raw(3, 3, 9, Y, nan_w, centre, o),
    }
    for name, run in cases.items():
        outs = fresh()
        assert run(outs) == 1, name                                     # BLUEST_ERR_ARG
        assert _lib.lib().bluest_last_error(), name
        assert all((o == -7.0).all() for o in outs), name
    assert _lib.lib().bluest_field_pilot_scratch(-1, None) == 1
    outs = fresh()
    assert raw(3, 3, 9, Y, w, centre, outs) == 0 and all_same(outs, expected(3, 3, 9))

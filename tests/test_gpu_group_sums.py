"""
GPU tests of bluest_group_sums (include/bluest_hip.h Part 11, csrc/gsums.hip) at its ABI: the bits of the numpy restatement of the
documented summation order (tests/gsums_ref.py) over every chunk edge, group width and load alignment; independent of the other
segments of the call, of the segment's position, of host or device memory and of the slab size; mu in the stated fma order;
inside the rounding bound of a long-double sum; strict about its arguments.
"""
import ctypes

import numpy as np
import pytest

import gsums_ref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

CHUNK = 128
COUNTS = (1, 127, 128, 129, 389)
ERR_ARG = 1


def data(n_out, N, L, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models: sums whose bits depend on the order of the additions"""
    rng = np.random.RandomState(seed)
    return 1.5 + 10.0 ** rng.uniform(-3, 3, L) * rng.randn(n_out, N, L)


def raw(segs, weights=None, repeat_of=None, R=0, override=None):
    """the raw call on a list of host arrays / CUDA tensors [n_out, N, L]: (rc, sums [n_out, T], mu or None)"""
    from bluest_amd import _lib
    S = len(segs)
    n_out = int(segs[0].shape[0])
    counts = np.array([int(v.shape[1]) for v in segs], dtype=np.int64)
    sizes = np.array([int(v.shape[2]) for v in segs], dtype=np.int32)
    ptrs = (ctypes.c_void_p * S)(*[_lib.ptr(v) for v in segs])
    T = int(sizes.sum())
    sums = np.full((n_out, T), -7.0)
    mu = None if weights is None else np.full((R, n_out), -7.0)
    rep = None if repeat_of is None else np.asarray(repeat_of, dtype=np.int64)
    args = dict(S=S, n_out=n_out, counts=_lib.ptr(counts), sizes=_lib.ptr(sizes), values=ctypes.cast(ptrs, ctypes.c_void_p),
                weights=_lib.ptr(weights), R=R, repeat_of=_lib.ptr(rep), sums=_lib.ptr(sums), mu=_lib.ptr(mu), stream=None)
    for k, v in (override or {}).items():                              # an argument of the call replaced as it is
        args[k] = _lib.ptr(v) if isinstance(v, np.ndarray) else v
    rc = _lib.lib().bluest_group_sums(*[args[k] for k in ("S", "n_out", "counts", "sizes", "values", "weights", "R", "repeat_of",
                                                           "sums", "mu", "stream")])
    return rc, sums, mu


def split(sums, segs):
    out, c = [], 0
    for v in segs:
        out.append(sums[:, c:c + v.shape[2]])
        c += v.shape[2]
    return out


@pytest.fixture(scope="module")
def pool():
    """70 ragged segments and the restatement's sums of each, computed once: counts around every chunk edge, a zero count in the
    middle, widths 1..64, three outputs"""
    rng = np.random.RandomState(70)
    widths = [1, 2, 3, 5, 32, 64] + rng.randint(1, 12, size=64).tolist()
    counts = list(COUNTS) + [0] + rng.randint(1, 40, size=28).tolist() + [0] + rng.randint(1, 300, size=35).tolist()
    segs = [data(3, N, L, 1000 + i) for i, (N, L) in enumerate(zip(counts, widths))]
    return segs, [gsums_ref.segment_sums(v) for v in segs]


@pytest.mark.parametrize("n_out", [1, 3])
@pytest.mark.parametrize("L", [1, 2, 3, 5, 32, 64])
def test_bits_of_the_restatement_at_every_chunk_edge(L, n_out):
    segs = [data(n_out, N, L, 7 * L + N) for N in COUNTS]
    rc, sums, _ = raw(segs)
    assert rc == 0
    for v, got in zip(segs, split(sums, segs)):
        assert same_bits(got, gsums_ref.segment_sums(v)), (L, n_out, v.shape[1])
    rc1, alone, _ = raw(segs[-1:])                                      # S = 1
    assert rc1 == 0 and same_bits(alone, split(sums, segs)[-1])


def test_more_chunks_than_fold_lanes():
    """65 and 130 chunks: the fold's lanes take a second and a third chunk each"""
    segs = [data(2, 64 * CHUNK + 77, 3, 1), data(2, 129 * CHUNK + 1, 2, 2)]
    rc, sums, _ = raw(segs)
    assert rc == 0
    for v, got in zip(segs, split(sums, segs)):
        assert same_bits(got, gsums_ref.segment_sums(v))


def test_seventy_segments_host_and_device_mixed(pool):
    import torch
    segs, want = pool
    mixed = [torch.from_numpy(v).cuda() if i % 3 == 1 and v.shape[1] > 0 else v for i, v in enumerate(segs)]
    torch.cuda.synchronize()
    rc, sums, _ = raw(mixed)
    assert rc == 0
    for i, (w, got) in enumerate(zip(want, split(sums, segs))):
        assert same_bits(got, w), (i, segs[i].shape)
    zero = [i for i, v in enumerate(segs) if v.shape[1] == 0]
    assert len(zero) == 2 and all((split(sums, segs)[i] == 0).all() and not np.signbit(split(sums, segs)[i]).any() for i in zero)
    rc2, again, _ = raw(mixed)
    assert rc2 == 0 and same_bits(again, sums)


def test_a_segment_keeps_its_bits_alone_in_a_batch_and_at_another_position(pool):
    import torch
    segs, want = pool
    for i in (4, 3, 40, 69):
        v = segs[i]
        rc, alone, _ = raw([v])
        assert rc == 0 and same_bits(alone, want[i])
        others = [segs[j] for j in (0, 8, 50)]
        for order in ([v] + others, others + [v], others[:2] + [v] + others[2:]):
            rc, sums, _ = raw(order)
            assert rc == 0 and same_bits(split(sums, order)[[k for k, o in enumerate(order) if o is v][0]], want[i])
        # from device memory, at a base that is 8- but not 16-byte aligned
        flat = torch.zeros(v.size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = torch.from_numpy(v).reshape(-1)
        shifted = flat[1:].reshape(v.shape)
        torch.cuda.synchronize()
        assert shifted.data_ptr() % 16 == 8
        rc, dev, _ = raw([shifted])
        assert rc == 0 and same_bits(dev, want[i])


def test_a_tiny_slab_budget_gives_the_same_bits(pool):
    from bluest_amd import _lib
    segs, want = pool
    big = [data(2, 5 * CHUNK + 9, 7, 3), data(2, 3, 4, 4), data(2, 2 * CHUNK + 5, 9, 5)]
    rc, whole, _ = raw(big)
    lib, before = _lib.lib(), ctypes.c_int64(0)
    assert rc == 0 and lib.bluest_group_sums_slab(1, ctypes.byref(before)) == 0 and before.value == 256 << 20
    try:
        rc1, tiny, _ = raw(big)                                         # room for one chunk of the widest segment: 8 slabs
        assert lib.bluest_group_sums_slab(3 * CHUNK * 7 * 8 * 2 + 1000, None) == 0
        rc2, mid, _ = raw(big)                                          # the first segment ends in the middle of a slab
        rc3, many, _ = raw(segs[:30])
    finally:
        assert lib.bluest_group_sums_slab(before.value, None) == 0
    assert rc1 == 0 and rc2 == 0 and rc3 == 0
    assert same_bits(tiny, whole) and same_bits(mid, whole)
    assert all(same_bits(a, b) for a, b in zip(split(many, segs[:30]), want[:30]))
    for v, got in zip(big, split(whole, big)):
        assert same_bits(got, gsums_ref.segment_sums(v))
    from bluest_amd import estimator
    py = estimator.group_sums(big, slab_bytes=1)                        # the Python entry sets the budget for its call only
    assert all(same_bits(a, b) for a, b in zip(py, split(whole, big)))
    now = ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(0, ctypes.byref(now)) == 0 and now.value == before.value


def test_a_cancellation_column_pins_the_order():
    """1e16, 1, -1e16, 1, ...: the exact sum is N / 2, and which of the ones survive depends on the order of the additions"""
    N = 388
    v = np.ones((1, N, 2))
    v[0, 0::4, 0], v[0, 2::4, 0] = 1e16, -1e16
    v[0, :, 1] = np.random.RandomState(1).permutation(v[0, :, 0])
    rc, sums, _ = raw([v])
    want = gsums_ref.segment_sums(v)
    assert rc == 0 and same_bits(sums, want)
    assert want[0, 0] != N / 2                                          # (a sum that lost no 1 would pin nothing)


def test_mu_in_the_stated_fma_order(pool):
    segs, want = pool
    pick = [segs[i] for i in (0, 2, 5, 7, 3, 30, 31, 4)]                # a zero count among them
    T = sum(v.shape[2] for v in pick)
    W = np.random.RandomState(3).randn(3, T) * 10.0 ** np.random.RandomState(4).uniform(-2, 2, T)
    for repeat_of, R in (([0] * 8, 1), ([0, 0, 0, 1, 3, 3, 3, 3], 4), ([0, 1, 1, 1, 1, 2, 2, 2], 3)):
        rc, sums, mu = raw(pick, weights=W, repeat_of=repeat_of, R=R)
        ref_sums, ref_mu = gsums_ref.group_sums(pick, W, repeat_of, R)
        assert rc == 0 and same_bits(sums, np.concatenate(ref_sums, axis=1)) and same_bits(mu, ref_mu), repeat_of
    assert (mu[:, :] != 0).all()
    rc, sums, mu = raw(pick, weights=W, repeat_of=[0, 0, 0, 1, 3, 3, 3, 3], R=4)
    assert rc == 0 and (mu[2] == 0).all()                               # a repeat without segments
    from bluest_amd import estimator
    out, py = estimator.group_sums(pick, weights=W, repeat_of=[0, 1, 1, 1, 1, 2, 2, 2])
    assert same_bits(py, ref_mu) and all(same_bits(a, b) for a, b in zip(out, ref_sums))


def test_sums_are_inside_the_rounding_bound(pool):
    segs, _ = pool
    rc, sums, _ = raw(segs)
    assert rc == 0
    worst = 0.0
    for v, got in zip(segs, split(sums, segs)):
        exact, absolute = gsums_ref.sums_ld(v)
        bound = (2 * v.shape[1] * gsums_ref.U * absolute).astype(np.float64)
        err = np.abs(got.astype(gsums_ref.LD) - exact).astype(np.float64)
        assert (err <= bound).all()
        worst = max(worst, float((err[bound > 0] / bound[bound > 0]).max()) if (bound > 0).any() else 0.0)
    print("largest error / bound:", worst)


def test_argument_errors():
    from bluest_amd import _lib
    lib = _lib.lib()
    a, b = np.ones((1, 4, 3)), 2 * np.ones((1, 2, 2))
    W = np.ones((1, 5))
    rc, sums, mu = raw([a, b], weights=W, repeat_of=[0, 1], R=2)
    assert rc == 0 and sums.tolist() == [[4.0, 4.0, 4.0, 4.0, 4.0]] and mu.tolist() == [[12.0], [8.0]]
    i64, i32 = (lambda *x: np.array(x, dtype=np.int64)), (lambda *x: np.array(x, dtype=np.int32))
    bad = {"S = 0": dict(S=0), "S < 0": dict(S=-1), "n_out = 0": dict(n_out=0), "n_out = 1025": dict(n_out=1025),
           "counts": dict(counts=None), "sizes": dict(sizes=None), "values": dict(values=None), "sums": dict(sums=None),
           "size 0": dict(sizes=i32(3, 0)), "size 65": dict(sizes=i32(65, 2)), "negative count": dict(counts=i64(4, -1)),
           "decreasing repeat_of": dict(repeat_of=i64(1, 0)), "repeat_of out of range": dict(repeat_of=i64(0, 2)),
           "repeat_of < 0": dict(repeat_of=i64(-1, 0)), "weights without mu": dict(mu=None), "mu without weights": dict(weights=None),
           "weights without repeat_of": dict(repeat_of=None), "R = 0": dict(R=0),
           "null segment": dict(values=ctypes.cast((ctypes.c_void_p * 2)(_lib.ptr(a), None), ctypes.c_void_p))}
    for what, change in bad.items():
        rc, s2, m2 = raw([a, b], weights=W, repeat_of=[0, 1], R=2, override=change)
        assert rc == ERR_ARG, what
        assert len(lib.bluest_last_error()) > 0, what
        assert (s2 == -7.0).all() and (m2 is None or (m2 == -7.0).all()), what          # a refused call writes nothing
    assert lib.bluest_group_sums_slab(-1, None) == ERR_ARG
    empty = np.ones((1, 0, 3))
    rc, sums, _ = raw([empty])                                          # no sample at all: zeros
    assert rc == 0 and (sums == 0).all()

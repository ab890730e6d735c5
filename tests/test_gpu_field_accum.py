"""
GPU tests of the resumable accumulator (include/bluest_hip.h Part 19, csrc/field_accum.hip, bluest_amd.field_stream.FieldAccumulator):
whatever the sequence of updates -- everything at once, row by row, a list of awkward sizes with host and device batches in turn,
host batches under a staging budget of one chunk, a device base that is not 16-byte aligned -- finish returns, compared as uint64,
the bits of the one-shot calls on the concatenation and of the numpy restatement of the streamed order (tests/field_accum_ref.py),
at every (L, d) at which a partial kernel takes another shape and at every count at which the tail and the lanes behave
differently.  NaN and Inf propagate as in the one-shot calls, an accumulator without coefficients launches no moment kernel, two
handles do not see each other, the state does not grow over a steady run, and the error codes are those of the header.
"""
import ctypes

import numpy as np
import pytest

import field_accum_ref as aref
import field_moments_ref as mref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

# (L, d): (1, 1), (3, 5), (64, 63) k_fmom_staged with sb = 128, 128 and 1; (2, 70) k_fmom_wide; (16, 64), (16, 1000) a workgroup per class
SHAPES = [(1, 1), (3, 5), (64, 63), (2, 70), (16, 64), (16, 1000)]
COUNTS = [0, 1, 127, 128, 129, 300]
BIG = 65 * 128 + 37                 # lanes 0 and 1 take a second chunk, and a tail remains
ERR_ARG, ERR_STATE = 1, 4
_cache = {}


def case(L, d, N):
    """(values, coef, one-shot sums, zsum, zsq on the GPU, the restatement's), computed once"""
    key = (L, d, N)
    if key not in _cache:
        from bluest_amd.field_errors import field_weighted_moments
        from bluest_amd.fields import field_group_sums
        v, coef = mref.data26(N, L, d, seed=1000 * L + 10 * d + N, signed=bool(N % 2))
        sums = field_group_sums([v])[0]
        _, zsum, zsq = field_weighted_moments([v], coef)[0]
        acc = aref.FieldAccumRef(L, d, coef, exact_products=True)
        acc.update(v)
        want = acc.finish()
        for a in (v, coef, sums, zsum, zsq):
            a.setflags(write=False)
        _cache[key] = (v, coef, sums, zsum, zsq, want)
    return _cache[key]


def run(v, coef, pieces, slab_bytes=None):
    """pieces: [(rows, on the device?)] in order"""
    import torch
    from bluest_amd.field_stream import FieldAccumulator
    kw = {} if slab_bytes is None else {"slab_bytes": slab_bytes}
    with FieldAccumulator(v.shape[1], v.shape[2], coef, **kw) as acc:
        at = 0
        for n, device in pieces:
            piece = np.array(v[at:at + n])
            acc.update(torch.from_numpy(piece).cuda() if device else piece)
            at += n
        assert at == v.shape[0]
        info = acc.info()
        return acc.finish(), info


def mixed(N):
    sizes, left = [], N
    for n in [1, 126, 1, 128, 300, 0, 127]:
        sizes.append(min(n, left))
        left -= sizes[-1]
    sizes.append(left)
    return [(n, bool(i % 2)) for i, n in enumerate(sizes)]


def check(L, d, N, pieces, **kw):
    v, coef, sums, zsum, zsq, want = case(L, d, N)
    (count, s, a, b), info = run(v, coef, pieces, **kw)
    assert count == N == want[0]
    for got, one_shot, restated in ((s, sums, want[1]), (a, zsum, want[2]), (b, zsq, want[3])):
        assert same_bits(got, one_shot) and same_bits(got, restated), (L, d, N, pieces[:4])
    return info


@pytest.mark.parametrize("L,d", SHAPES)
@pytest.mark.parametrize("N", COUNTS)
def test_any_sequence_of_updates_gives_the_bits_of_the_one_shot_calls(L, d, N):
    check(L, d, N, [(N, True)])
    check(L, d, N, [(N, False)])
    if N <= 130:
        check(L, d, N, [(1, bool(i % 3)) for i in range(N)])
    check(L, d, N, mixed(N))
    info = check(L, d, N, [(N, False)], slab_bytes=1)                   # a staging budget of one chunk
    assert info[0] == N and info[1] == N // 128 and info[2] == N % 128
    if N in (0, 1):
        zs = run(*case(L, d, N)[:2], [(N, True)])[0]
        assert all((x == 0).all() and not np.signbit(x).any() for x in zs[2:]) and (N == 1 or not np.signbit(zs[1]).any())


@pytest.mark.parametrize("L,d", [(3, 5), (16, 64)])
def test_lanes_take_a_second_chunk_and_a_tail_remains(L, d):
    check(L, d, BIG, [(BIG, True)])
    check(L, d, BIG, [(500, True)] * 16 + [(357, True)])
    check(L, d, BIG, mixed(BIG))
    info = check(L, d, BIG, [(64 * 128 + 100, False), (65, False)], slab_bytes=1)
    assert info[1] == 65 and info[2] == 37


def test_a_device_base_that_is_not_16_byte_aligned():
    import torch
    from bluest_amd.field_stream import FieldAccumulator
    for L, d in [(3, 5), (2, 70), (16, 64)]:
        v, coef, sums, zsum, zsq, _ = case(L, d, 300)
        flat = torch.empty(v.size + 1, dtype=torch.float64, device="cuda")
        flat[1:] = torch.from_numpy(np.array(v).reshape(-1)).cuda()
        dev = flat[1:].view(300, L, d)
        assert dev.data_ptr() % 16 == 8
        with FieldAccumulator(L, d, coef) as acc:
            acc.update(dev[:131])
            acc.update(dev[131:])
            count, s, a, b = acc.finish()
        assert count == 300 and same_bits(s, sums) and same_bits(a, zsum) and same_bits(b, zsq)


@pytest.mark.parametrize("L,d", [(3, 5), (2, 70), (16, 64)])
def test_nan_and_inf_propagate_as_in_the_one_shot_calls(L, d):
    from bluest_amd.field_errors import field_weighted_moments
    from bluest_amd.fields import field_group_sums
    rng = np.random.RandomState(L + d)
    coef = rng.randn(L)
    for where in ("middle", "first"):
        v = 1.5 + rng.randn(300, L, d)
        row = 0 if where == "first" else 200
        v[row, 0, 0], v[row, L - 1, d - 1] = np.nan, np.inf
        v[150, 0, d - 1] = -np.inf
        sums = field_group_sums([v])[0]
        _, zsum, zsq = field_weighted_moments([v], coef)[0]
        for pieces in ([(300, True)], mixed(300)):
            (count, s, a, b), _ = run(v, coef, pieces)
            assert count == 300 and same_bits(s, sums) and same_bits(a, zsum) and same_bits(b, zsq)
        assert np.isnan(sums[0, 0]) and np.isnan(zsum[0]) and np.isfinite(sums[0, 1]) and np.isinf(sums[0, d - 1])


def test_without_coefficients_no_moment_kernel_is_launched():
    from bluest_amd import _lib
    v, coef, sums, _, _, _ = case(3, 5, 300)
    (count, s, a, b), info = run(v, None, mixed(300))
    assert count == 300 and same_bits(s, sums) and a is None and b is None
    assert info[4] > 0 and info[5] == 0
    _, with_coef = run(v, coef, mixed(300))
    assert with_coef[5] == with_coef[4] > 0
    lib = _lib.lib()
    h, n = ctypes.c_void_p(), ctypes.c_int64(0)
    out, z = np.full((3, 5), -7.0), np.full(5, -7.0)
    assert lib.bluest_field_accum_create(3, 5, None, ctypes.byref(h), None) == 0
    try:
        assert lib.bluest_field_accum_finish(h, ctypes.byref(n), _lib.ptr(out), _lib.ptr(z), _lib.ptr(z), None) == ERR_ARG    # zsum without coef
        assert (out == -7.0).all() and lib.bluest_field_accum_finish(h, ctypes.byref(n), _lib.ptr(out), None, None, None) == 0
        assert n.value == 0 and (out == 0).all() and not np.signbit(out).any()
    finally:
        lib.bluest_field_accum_destroy(h)


def test_the_error_codes():
    from bluest_amd import _lib
    lib = _lib.lib()
    v, coef = np.ones((4, 3, 5)), np.ones(3)
    h, n = ctypes.c_void_p(), ctypes.c_int64(-7)
    out, z, zz = np.full((3, 5), -7.0), np.full(5, -7.0), np.full(5, -7.0)
    assert lib.bluest_field_accum_create(3, 5, _lib.ptr(coef), ctypes.byref(h), None) == 0
    try:
        upd = lambda rows, p: lib.bluest_field_accum_update(h, rows, p, None)
        fin = lambda a, b, c, d: lib.bluest_field_accum_finish(h, a, b, c, d, None)
        assert upd(-1, _lib.ptr(v)) == ERR_ARG and upd(4, None) == ERR_ARG and upd(3, _lib.ptr(v) + 4) == ERR_ARG
        assert upd(0, None) == 0 and upd(4, _lib.ptr(v)) == 0
        assert fin(None, _lib.ptr(out), _lib.ptr(z), _lib.ptr(zz)) == ERR_ARG and fin(ctypes.byref(n), None, _lib.ptr(z), _lib.ptr(zz)) == ERR_ARG
        assert fin(ctypes.byref(n), _lib.ptr(out), _lib.ptr(z), None) == ERR_ARG and fin(ctypes.byref(n), _lib.ptr(out), None, _lib.ptr(zz)) == ERR_ARG
        assert fin(ctypes.byref(n), _lib.ptr(out), None, None) == ERR_ARG                # coef without zsum
        assert n.value == -7 and (out == -7.0).all() and (z == -7.0).all()               # nothing was written, nothing changed
        assert fin(ctypes.byref(n), _lib.ptr(out), _lib.ptr(z), _lib.ptr(zz)) == 0
        assert n.value == 4 and (out == 4.0).all() and (z == 0).all() and (zz == 0).all()
        assert upd(4, _lib.ptr(v)) == ERR_STATE and fin(ctypes.byref(n), _lib.ptr(out), _lib.ptr(z), _lib.ptr(zz)) == ERR_STATE
    finally:
        assert lib.bluest_field_accum_destroy(h) == 0


def test_two_handles_interleaved_give_what_each_gives_alone():
    from bluest_amd.field_stream import FieldAccumulator
    import torch
    va, ca, sa, za, qa, _ = case(3, 5, 300)
    vb, cb, sb, zb, qb, _ = case(16, 64, 300)
    with FieldAccumulator(3, 5, ca) as a, FieldAccumulator(16, 64, cb) as b:
        for lo in range(0, 300, 70):
            a.update(np.array(va[lo:lo + 70]))
            b.update(torch.from_numpy(np.array(vb[lo:lo + 70])).cuda())
        got_b, got_a = b.finish(), a.finish()
    assert same_bits(got_a[1], sa) and same_bits(got_a[2], za) and same_bits(got_a[3], qa)
    assert same_bits(got_b[1], sb) and same_bits(got_b[2], zb) and same_bits(got_b[3], qb)


def test_a_steady_run_of_equal_batches_does_not_allocate():
    import torch
    from bluest_amd.field_stream import FieldAccumulator
    rng = np.random.RandomState(0)
    batch = torch.from_numpy(rng.randn(500, 3, 64)).cuda()
    with FieldAccumulator(3, 64, np.ones(3)) as acc:
        seen = []
        for _ in range(12):
            acc.update(batch)
            seen.append(acc.info())
        assert seen[-1][0] == 6000 and seen[-1][3] == seen[2][3] and seen[-1][6] == seen[2][6]
        fixed = (64 * 3 * 64 + 64 * 2 * 64 + 3 * 64 + 128 * 3 * 64) * 8
        assert fixed <= seen[-1][6] <= fixed + 8 * 500 * 3 * 64                # the state: about 192 rows and a scratch below one batch

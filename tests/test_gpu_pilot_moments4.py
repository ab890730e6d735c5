"""
GPU tests of bluest_pilot_moments4 (include/bluest_hip.h Part 14, csrc/pilot4.hip) at its ABI and of its wrapper
bluest_amd.pilot_errors.pilot_fourth_moments: every sum within the derived rounding bound of the long-double restatement
(tests/pilot4_ref.py) at the shapes where the kernel takes another path, the same bits however the data arrives, hard inputs, and
strict arguments.

Shapes: L = 1 has no off-diagonal pair, L = 2 the half diagonal, L = 33 half-waves that straddle two diagonals, L = 64 nine
pairs per thread; the N sit at the chunk edges (128) and include a third, short chunk.
"""
import numpy as np
import pytest

import pilot4_ref
from pilot4_ref import LD

pytestmark = pytest.mark.gpu

CHUNK = 128
NAMES = ("first", "s11", "s21", "s22", "tpow")


def moments4(values, shift=None, differences=True, N=None, L=None, n_out=None, outputs=None):
    """the raw call on a host array or a CUDA tensor: (rc, first, s11, s21, s22, tpow), outputs pre-filled with -7.0"""
    from bluest_amd import _lib
    shape = tuple(values.shape)
    if outputs is None:
        outputs = [np.full((shape[0], shape[2]), -7.0)] + [np.full((shape[0], shape[2], shape[2]), -7.0) for _ in range(3)]
        outputs.append(np.full((shape[0], 4, shape[2], shape[2]), -7.0) if differences else None)
    n_out, N, L = (shape[0] if n_out is None else n_out, shape[1] if N is None else N, shape[2] if L is None else L)
    rc = _lib.lib().bluest_pilot_moments4(N, L, n_out, _lib.ptr(values), _lib.ptr(shift), *[_lib.ptr(o) for o in outputs], None)
    return (rc,) + tuple(outputs)


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


def all_same(xs, ys):
    return all((a is None and b is None) or same_bits(a, b) for a, b in zip(xs, ys))


def real_data(n_out, N, L, seed):
    """mean 1.5, scales from 1e-2 to 1e2 across the models, and models 0 and 1 differing by 1e-6"""
    rng = np.random.RandomState(seed)
    scale = 10.0 ** rng.uniform(-2, 2, L)
    scale[0] = 1.0
    Y = 1.5 + scale * rng.randn(n_out, N, L)
    if L > 1:
        Y[:, :, 1] = Y[:, :, 0] + 1e-6 * rng.randn(n_out, N)
    return Y


def check_within(got, values, shift=None, what=()):
    """every sum within (N + 16) u sum|term| of the long-double value; returns the largest error / bound"""
    differences = got[4] is not None
    ref, bound = pilot4_ref.sums_ld(values, shift, differences), pilot4_ref.bounds(values, shift, differences)
    worst = 0.0
    for name, g, r, b in zip(NAMES, got, ref, bound):
        if g is None:
            continue
        err = np.abs(g.astype(LD) - r).astype(np.float64)
        assert (err <= b).all(), (name, what, float((err[b > 0] / b[b > 0]).max()) if (b > 0).any() else err.max())
        if (b > 0).any():
            worst = max(worst, float((err[b > 0] / b[b > 0]).max()))
    return worst


@pytest.mark.parametrize("L", [1, 2, 3, 33, 64])
def test_every_sum_within_the_bound_at_every_shape(L):
    outside = ~np.triu(np.ones((L, L), dtype=bool), 1)
    worst = 0.0
    for N in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 300):
        Y = real_data(3, N, L, 1000 * L + N)
        rc, *batch = moments4(Y)
        assert rc == 0
        worst = max(worst, check_within(batch, Y, what=(L, N, 3)))
        rc, *alone = moments4(np.ascontiguousarray(Y[:1]))              # one output alone: the bits it has inside the batch
        assert rc == 0 and all_same(alone, [b[:1] for b in batch]), (L, N)
        first, s11, s21, s22, tpow = batch
        assert same_bits(s11, s11.transpose(0, 2, 1)) and same_bits(s22, s22.transpose(0, 2, 1))
        assert same_bits(tpow[:, :, outside], np.zeros((3, 4, int(outside.sum()))))      # +0.0 outside i < j
        if N == 1:                                                      # d and t are exactly 0
            assert all(same_bits(x, np.zeros_like(x)) for x in batch)
    print("L = %d: largest error / bound %.3f" % (L, worst))


def test_host_and_device_input_two_runs_and_a_null_tpow_give_the_same_bits():
    import torch
    from bluest_amd import pilot_errors
    Y = real_data(2, 2 * CHUNK + 9, 20, 8)
    rc, *host = moments4(Y)
    rc2, *again = moments4(Y)
    assert rc == 0 and rc2 == 0 and all_same(host, again)
    T = torch.from_numpy(Y).cuda()
    torch.cuda.synchronize()
    rc3, *dev = moments4(T)
    assert rc3 == 0 and all_same(host, dev)
    rc4, *plain = moments4(Y, differences=False)
    assert rc4 == 0 and plain[4] is None and all_same(host[:4], plain[:4])
    for values in (Y, T):                                               # the wrapper: both kinds of input, with and without tpow
        used, *got = pilot_errors.pilot_fourth_moments(values)
        assert same_bits(used, Y[:, 0, :]) and all_same(host, got)
        used, *got = pilot_errors.pilot_fourth_moments(values, differences=False)
        assert got[4] is None and all_same(host[:4], got[:4])


def test_an_explicit_first_sample_shift_gives_the_bits_of_a_null_shift():
    Y = real_data(3, CHUNK + 40, 33, 9)
    rc, *null = moments4(Y)
    rc2, *explicit = moments4(Y, shift=np.ascontiguousarray(Y[:, 0, :]))
    assert rc == 0 and rc2 == 0 and all_same(null, explicit)
    shift = np.ascontiguousarray(Y[:, 5, :] + 0.25)                     # any other shift: the sums change, the bound holds
    rc3, *moved = moments4(Y, shift=shift)
    assert rc3 == 0 and not same_bits(moved[1], null[1])
    check_within(moved, Y, shift)


def test_a_slabbed_host_call_adds_the_slabs_in_order():
    from bluest_amd import pilot_errors
    n_out, N, L = 2, 3 * CHUNK + 5, 9
    Y = real_data(n_out, N, L, 10)
    shift = np.ascontiguousarray(Y[:, 0, :])
    whole = pilot_errors.pilot_fourth_moments(Y)
    for slab_bytes, per_slab in ((1, CHUNK), (L * 8 * (2 * CHUNK + 17), 2 * CHUNK)):
        used, *split = pilot_errors.pilot_fourth_moments(Y, slab_bytes=slab_bytes)
        assert same_bits(used, shift)
        by_hand = []
        for n in range(n_out):
            total = None
            for start in range(0, N, per_slab):
                rc, *part = moments4(np.ascontiguousarray(Y[n:n + 1, start:start + per_slab]), shift=shift[n:n + 1])
                assert rc == 0
                total = part if total is None else [t + p for t, p in zip(total, part)]
            by_hand.append(total)
        by_hand = [np.concatenate(parts, axis=0) for parts in zip(*by_hand)]
        assert all_same(split, by_hand), slab_bytes
        check_within(split, Y)                                          # one more addition per slab: inside the slack of 16
    check_within(whole[1:], Y)


def test_a_large_mean_costs_nothing():
    """mean 1e8 over unit variance: y and the first sample agree to a factor of two, so d = y - a is exact and the standard errors
    agree with the two-pass long-double ones to 1e-12 relative"""
    from bluest_amd import pilot_errors
    rng = np.random.RandomState(11)
    N, L = 300, 3
    Y = 1e8 + rng.randn(1, N, L) @ np.array([[1.0, 0.8, 0.3], [0.0, 0.6, 0.5], [0.0, 0.0, 0.7]])
    _, first, s11, s21, s22, tpow = pilot_errors.pilot_fourth_moments(Y)
    se_c, se_d = pilot_errors.pilot_standard_errors(N, first, s11, s21, s22, tpow)
    ref_c, ref_d = pilot4_ref.standard_errors(Y)
    iu = np.triu_indices(L, 1)
    print("relative error of SE(C):", np.abs(se_c / ref_c - 1).max(), "of SE(dV):", np.abs(se_d[0][iu] / ref_d[0][iu] - 1).max())
    assert np.abs(se_c / ref_c - 1).max() <= 1e-12
    assert np.abs(se_d[0][iu] / ref_d[0][iu] - 1).max() <= 1e-12
    assert np.isnan(se_d[0][np.tril_indices(L)]).all()


def test_two_nearly_equal_models_keep_their_difference_moments():
    """models 0 and 1 of real_data differ by 1e-6: tpow comes from the explicit differences and stays within the bound, which for
    the even powers (positive terms) is (N + 16) u < 1e-12 relative.  Formed from the pair sums instead, sum t^2 = s11[0,0] -
    2 s11[0,1] + s11[1,1] is a difference of terms of size N against a result of size N 1e-12: three digits are left of it
    (off by 9.5e-4 on an MI355X, where tpow is off by 3e-16), and of sum t^4 (size N 1e-24, from s22 and its kin) none."""
    N, L = 300, 8
    Y = real_data(1, N, L, 12)
    rc, first, s11, s21, s22, tpow = moments4(Y)
    assert rc == 0
    check_within((first, s11, s21, s22, tpow), Y)
    exact = float(pilot4_ref.sums_ld(Y)[4][0, 3, 0, 1])
    exact2 = float(pilot4_ref.sums_ld(Y)[4][0, 1, 0, 1])
    route2 = s11[0, 0, 0] - 2 * s11[0, 0, 1] + s11[0, 1, 1]
    print("sum t^2: kernel off by %.2e, pair-sum route off by %.2e; sum t^4: kernel off by %.2e"
          % (abs(tpow[0, 1, 0, 1] / exact2 - 1), abs(route2 / exact2 - 1), abs(tpow[0, 3, 0, 1] / exact - 1)))
    assert abs(tpow[0, 1, 0, 1] / exact2 - 1) <= 1e-12 and abs(tpow[0, 3, 0, 1] / exact - 1) <= 1e-12
    assert abs(route2 / exact2 - 1) > 1e-6


def test_nan_and_inf_propagate():
    Y = real_data(2, CHUNK + 3, 5, 13)
    Y[1, CHUNK + 1, 2] = np.nan
    rc, first, s11, s21, s22, tpow = moments4(Y)
    assert rc == 0
    assert np.isfinite(first[0]).all() and np.isfinite(s22[0]).all() and np.isfinite(tpow[0]).all()      # output 0 is untouched
    assert np.isnan(first[1, 2]) and np.isnan(s11[1, 2]).all() and np.isnan(s21[1, :, 2]).all() and np.isnan(s22[1, :, 2]).all()
    assert np.isnan(tpow[1, :, 0, 2]).all() and np.isnan(tpow[1, :, 2, 4]).all() and np.isfinite(tpow[1, :, 0, 1]).all()
    assert np.isfinite(np.delete(first[1], 2)).all()
    Y[1, CHUNK + 1, 2] = np.inf
    rc, first, s11, s21, s22, tpow = moments4(Y)
    assert rc == 0 and first[1, 2] == np.inf and s22[1, 2, 2] == np.inf and not np.isfinite(tpow[1, 0, 0, 2])


def test_refused_calls_write_nothing_and_a_good_call_follows():
    from bluest_amd import _lib
    lib = _lib.lib()
    Y = np.ones((1, 4, 3))
    Y[0, :, 1] = [1.0, 2.0, 3.0, 4.0]
    outs = [np.full((1, 3), -7.0)] + [np.full((1, 3, 3), -7.0) for _ in range(3)] + [np.full((1, 4, 3, 3), -7.0)]
    p = _lib.ptr
    good = [4, 3, 1, p(Y), None] + [p(o) for o in outs] + [None]
    bad = {"L = 0": {1: 0}, "L = 65": {1: 65}, "n_out = 0": {2: 0}, "n_out = 1025": {2: 1025}, "N = 0": {0: 0}, "N < 0": {0: -3},
           "chunks": {0: 128 * 2**31 + 1}, "values": {3: None}, "first": {5: None}, "s11": {6: None}, "s21": {7: None}, "s22": {8: None}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items(): args[k] = v
        assert lib.bluest_pilot_moments4(*args) == 1, what              # BLUEST_ERR_ARG
        assert len(lib.bluest_last_error()) > 0, what
        assert all((o == -7.0).all() for o in outs), what               # before anything is written
    assert lib.bluest_pilot_moments4(*good) == 0
    first, s11, s21, s22, tpow = outs
    assert first.tolist() == [[0.0, 6.0, 0.0]] and s11[0, 1, 1] == 14.0 and s21[0, 1, 1] == 36.0 and s22[0, 1, 1] == 98.0
    assert tpow[0, :, 0, 1].tolist() == [-6.0, 14.0, -36.0, 98.0] and tpow[0, :, 1, 2].tolist() == [6.0, 14.0, 36.0, 98.0]
    assert not tpow[0, :, 1, 0].any() and not tpow[0, :, 0, 2].any()

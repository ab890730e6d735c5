"""
GPU tests of bluest_pilot_stats (include/bluest_hip.h Part 10, csrc/pilot.hip) at its ABI: exact on integer data (every sum is
then exact in float64 in any order, so the pair map, the chunk edges, the fold and the mirror are pinned bit for bit), within
the derived rounding bounds of the long-double sums on real data, deterministic, and strict about its arguments.
"""

import numpy as np
import pytest

import pilot_ref

pytestmark = pytest.mark.gpu

CHUNK = 128
U = 2.0 ** -53


def stats(values, N=None, L=None, n_out=None, differences=True):
    """the raw call on a host array or a CUDA tensor: (rc, sumse, sumsc, sumsd1, sumsd2)"""
    from bluest_amd import _lib
    shape = tuple(values.shape)
    n_out, N, L = (shape[0] if n_out is None else n_out, shape[1] if N is None else N, shape[2] if L is None else L)
    se, sc = np.full((shape[0], shape[2]), -7.0), np.full((shape[0], shape[2], shape[2]), -7.0)
    d1 = np.full_like(sc, -7.0) if differences else None
    d2 = np.full_like(sc, -7.0) if differences else None
    rc = _lib.lib().bluest_pilot_stats(N, L, n_out, _lib.ptr(values), _lib.ptr(se), _lib.ptr(sc), _lib.ptr(d1), _lib.ptr(d2), None)
    return rc, se, sc, d1, d2


def int_sums(Y):
    Y = Y.astype(np.int64)
    D = Y[:, :, :, None] - Y[:, :, None, :]
    upper = np.triu(np.ones((Y.shape[2], Y.shape[2]), dtype=np.int64), 1)
    return Y.sum(axis=1), np.einsum("nsi,nsj->nij", Y, Y), D.sum(axis=1) * upper, (D * D).sum(axis=1) * upper


def same_bits(a, b):
    return np.array_equal(np.ascontiguousarray(a, dtype=np.float64).view(np.int64), np.ascontiguousarray(b, dtype=np.float64).view(np.int64))


@pytest.mark.parametrize("L", [1, 2, 3, 17, 63, 64])
def test_integer_data_is_exact(L):
    rng = np.random.RandomState(100 + L)
    for N in (1, 2, CHUNK - 1, CHUNK, CHUNK + 1, 3 * CHUNK + 5):
        for n_out in (1, 3):
            Y = rng.randint(-1000, 1001, size=(n_out, N, L)).astype(np.float64)
            rc, *got = stats(Y)
            assert rc == 0
            for name, g, want in zip(("sumse", "sumsc", "sumsd1", "sumsd2"), got, int_sums(Y)):
                assert same_bits(g, want.astype(np.float64)), (name, L, N, n_out, np.argwhere(g != want)[:4])


def real_data(N, L, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models, and models 0 and 1 differing by 1e-6"""
    rng = np.random.RandomState(seed)
    scale = 10.0 ** rng.uniform(-3, 3, L)
    scale[0] = 1.0
    Y = 1.5 + scale * rng.randn(2, N, L)
    if L > 1:
        Y[:, :, 1] = Y[:, :, 0] + 1e-6 * rng.randn(2, N)
    return Y


@pytest.mark.parametrize("N,L", [(517, 64), (129, 17), (4000, 8)])
def test_real_data_within_the_rounding_bounds(N, L):
    Y = real_data(N, L, N + L)
    rc, se, sc, d1, d2 = stats(Y)
    assert rc == 0
    le, lc, l1, l2 = pilot_ref.sums_ld(Y)
    ae, ac, a1, a2 = pilot_ref.abs_sums_ld(Y)
    upper = np.triu(np.ones((L, L)), 1)
    worst = {}
    for name, got, ref, bound in (("sumse", se, le, (N + 2) * U * ae), ("sumsc", sc, lc, (N + 2) * U * ac),
                                  ("sumsd1", d1, l1, (N + 4) * U * a1 * upper), ("sumsd2", d2, l2, (N + 4) * U * a2 * upper)):
        err, bound = np.abs(got.astype(pilot_ref.LD) - ref).astype(np.float64), np.asarray(bound, dtype=np.float64)
        worst[name] = float((err[bound > 0] / bound[bound > 0]).max())
        assert (err <= bound).all(), (name, worst[name])
    print("largest error / bound:", worst)
    assert (d1 * (1 - upper) == 0).all() and (d2 * (1 - upper) == 0).all() and same_bits(sc, sc.transpose(0, 2, 1))
    # why the kernel exists: the variance of the difference of the two close models, from the explicit differences and from
    # C_00 + C_11 - 2 C_01 of the same run
    for n in range(Y.shape[0]):
        exact = float(l2[n, 0, 1] / N - (l1[n, 0, 1] / N) ** 2)
        direct = d2[n, 0, 1] / N - (d1[n, 0, 1] / N) ** 2
        C = sc[n] / N - np.outer(se[n], se[n]) / N**2
        route = C[0, 0] + C[1, 1] - 2 * C[0, 1]
        print("output %d: dV %.17g, explicit differences off by %.2e, covariance route off by %.2e"
              % (n, exact, abs(direct / exact - 1), abs(route / exact - 1)))
        assert abs(direct / exact - 1) <= 1e-12
        assert abs(route / exact - 1) > 1e-6


def test_two_calls_give_identical_bits_and_null_differences_change_nothing():
    Y = real_data(3 * CHUNK + 5, 33, 7)
    rc, *first = stats(Y)
    rc2, *second = stats(Y)
    assert rc == 0 and rc2 == 0 and all(same_bits(a, b) for a, b in zip(first, second))
    rc3, se, sc, d1, d2 = stats(Y, differences=False)
    assert rc3 == 0 and d1 is None and d2 is None and same_bits(se, first[0]) and same_bits(sc, first[1])


def test_device_input_gives_the_bits_of_host_input():
    import torch
    from bluest_amd import pilot
    Y = real_data(2 * CHUNK + 9, 20, 8)
    rc, *host = stats(Y)
    T = torch.from_numpy(Y).cuda()
    torch.cuda.synchronize()
    rc2, *dev = stats(T)
    assert rc == 0 and rc2 == 0 and all(same_bits(a, b) for a, b in zip(host, dev))
    assert all(same_bits(a, b) for a, b in zip(host, pilot.pilot_statistics(T)))
    assert all(same_bits(a, b) for a, b in zip(host, pilot.pilot_statistics(Y)))
    se, sc, d1, d2 = pilot.pilot_statistics(Y, differences=False)
    assert d1 is None and d2 is None and same_bits(se, host[0]) and same_bits(sc, host[1])


def test_slab_split_equals_the_single_call_on_integer_data():
    from bluest_amd import pilot
    n_out, N, L = 2, 3 * CHUNK + 5, 9
    Y = np.random.RandomState(9).randint(-1000, 1001, size=(n_out, N, L)).astype(np.float64)
    whole = pilot.pilot_statistics(Y)
    for slab_bytes in (1, L * 8 * CHUNK, L * 8 * (2 * CHUNK + 17)):      # per output: 4 slabs, 4 slabs, 2 slabs
        split = pilot.pilot_statistics(Y, slab_bytes=slab_bytes)
        assert all(same_bits(a, b) for a, b in zip(whole, split)), slab_bytes
    assert all(same_bits(a, b.astype(np.float64)) for a, b in zip(whole, int_sums(Y)))


def test_argument_errors():
    from bluest_amd import _lib
    lib = _lib.lib()
    Y = np.ones((1, 4, 3))
    se, sc, d1, d2 = np.zeros((1, 3)), np.zeros((1, 3, 3)), np.zeros((1, 3, 3)), np.zeros((1, 3, 3))
    p = _lib.ptr
    good = (4, 3, 1, p(Y), p(se), p(sc), p(d1), p(d2), None)
    assert lib.bluest_pilot_stats(*good) == 0
    bad = {"L = 0": {1: 0}, "L = 65": {1: 65}, "n_out = 0": {2: 0}, "n_out = 1025": {2: 1025}, "N = 0": {0: 0}, "N < 0": {0: -3},
           "values": {3: None}, "sumse": {4: None}, "sumsc": {5: None}, "only sumsd1": {7: None}, "only sumsd2": {6: None}}
    for what, change in bad.items():
        args = list(good)
        for k, v in change.items(): args[k] = v
        assert lib.bluest_pilot_stats(*args) == 1, what                 # BLUEST_ERR_ARG
        assert len(lib.bluest_last_error()) > 0, what
    assert se[0, 0] == 4.0 and sc[0, 1, 2] == 4.0 and d1.max() == 0.0   # the good call's results, untouched by the refused ones

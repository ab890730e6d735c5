"""
GPU tests of bluest_field_stats (include/bluest_hip.h Part 12, csrc/fields.hip) at its ABI: exact on integer data, the bits of
bluest_pilot_stats at d = 1 and w = 1, the bits of the numpy restatement of the documented summation order (tests/fields_ref.py)
across chunk, tile and lane edges, the same from host and device memory and wherever a slab ends, inside the derived rounding
bounds of the long-double sums, and strict about its arguments.
"""
import ctypes

import numpy as np
import pytest

import fields_ref
import pilot_ref
from fields_ref import CHUNK, TILE, same_bits

pytestmark = pytest.mark.gpu

U = fields_ref.U
ERR_ARG = 1


def stats(values, w, differences=True, override=None):
    """the raw call on a host array or a CUDA tensor [N, L, d]: (rc, sumse [L, d], sumsc [L, L], sumsd1 [P, d], sumsd2 [L, L])"""
    from bluest_amd import _lib
    N, L, d = (int(x) for x in values.shape)
    P = L * (L - 1) // 2
    w = np.ascontiguousarray(w, dtype=np.float64)
    se, sc = np.full((L, d), -7.0), np.full((L, L), -7.0)
    d1 = np.full((max(P, 1), d), -7.0) if differences else None
    d2 = np.full((L, L), -7.0) if differences else None
    args = [N, L, d, _lib.ptr(values), _lib.ptr(w), _lib.ptr(se), _lib.ptr(sc), _lib.ptr(d1), _lib.ptr(d2), None]
    for k, v in (override or {}).items():
        args[k] = _lib.ptr(v) if isinstance(v, np.ndarray) else v
    rc = _lib.lib().bluest_field_stats(*args)
    return rc, se, sc, (d1[:P] if differences else None), d2


def real_data(N, L, d, seed):
    """mean 1.5, scales from 1e-3 to 1e3 across the models and from 0.1 to 10 across the components, models 0 and 1 differing by
    1e-6; weights between 0.01 and 100, one of them 0 when there are several"""
    rng = np.random.RandomState(seed)
    scale = 10.0 ** rng.uniform(-3, 3, (L, 1)) * 10.0 ** rng.uniform(-1, 1, d)
    scale[0] = 1.0
    Y = 1.5 + scale * rng.randn(N, L, d)
    if L > 1:
        Y[:, 1] = Y[:, 0] + 1e-6 * rng.randn(N, d)
    w = 10.0 ** rng.uniform(-2, 2, d)
    if d > 2:
        w[d // 2] = 0.0
    return Y, w


@pytest.mark.parametrize("L,d", [(1, 1), (2, 9), (3, 40), (17, 8), (33, 17), (64, 10)])
def test_integer_data_is_exact(L, d):
    """every sum is exact in float64 in any order: the pair map, the tile and chunk edges, the folds and the mirror are pinned"""
    rng = np.random.RandomState(100 * L + d)
    for N in (1, CHUNK, CHUNK + 1, 2 * CHUNK + 5):
        Y = rng.randint(-300, 301, size=(N, L, d)).astype(np.float64)
        w = rng.randint(0, 4, size=d).astype(np.float64)
        rc, se, sc, d1, d2 = stats(Y, w)
        assert rc == 0
        Z, wi = Y.astype(np.int64), w.astype(np.int64)
        D = Z[:, :, None, :] - Z[:, None, :, :]
        iu = fields_ref.pairs(L)
        upper = np.triu(np.ones((L, L), dtype=np.int64), 1)
        assert same_bits(se, Z.sum(axis=0).astype(np.float64)), (N, "sumse")
        assert same_bits(sc, np.einsum("sic,c,sjc->ij", Z, wi, Z).astype(np.float64)), (N, "sumsc")
        assert same_bits(d1, D.sum(axis=0)[iu[0], iu[1]].astype(np.float64)), (N, "sumsd1")
        assert same_bits(d2, (np.einsum("sijc,c,sijc->ij", D, wi, D) * upper).astype(np.float64)), (N, "sumsd2")


@pytest.mark.parametrize("N,L", [(1, 1), (14, 4), (CHUNK + 1, 64), (3 * CHUNK + 5, 33), (70 * CHUNK, 2)])
def test_one_component_with_weight_one_has_the_bits_of_the_pilot_statistics(N, L):
    from bluest_amd import _lib
    Y = pilot_ref_data(N, L, 11 * N + L)
    se, sc, d1, d2 = (np.full(s, -7.0) for s in ((1, L), (1, L, L), (1, L, L), (1, L, L)))
    assert _lib.lib().bluest_pilot_stats(N, L, 1, _lib.ptr(Y), _lib.ptr(se), _lib.ptr(sc), _lib.ptr(d1), _lib.ptr(d2), None) == 0
    rc, fe, fc, f1, f2 = stats(np.ascontiguousarray(Y[0][:, :, None]), [1.0])
    iu = fields_ref.pairs(L)
    assert rc == 0 and same_bits(fe[:, 0], se[0]) and same_bits(fc, sc[0]) and same_bits(f2, d2[0])
    assert same_bits(f1[:, 0], d1[0][iu[0], iu[1]])


def pilot_ref_data(N, L, seed):
    rng = np.random.RandomState(seed)
    Y = 1.5 + 10.0 ** rng.uniform(-3, 3, L) * rng.randn(1, N, L)
    if L > 1:
        Y[:, :, 1] = Y[:, :, 0] + 1e-6 * rng.randn(1, N)
    return Y


def fixture_values():
    g = pilot_ref.case("inner")
    return np.ascontiguousarray(np.stack(g["blocks"], axis=1)[0]), g["vec_weights"]


SHAPES = {"smallest": (1, 1, 1), "fixture": (14, 4, 3), "chunk and tile edge": (CHUNK + 1, 5, 2 * TILE + 1),
          "widest L": (3, 64, TILE + 1), "odd L": (130, 33, 2), "many tiles": (2, 2, 1000)}


@pytest.mark.parametrize("name", list(SHAPES))
def test_bits_of_the_restatement(name):
    N, L, d = SHAPES[name]
    Y, w = fixture_values() if name == "fixture" else real_data(N, L, d, N + L + d)
    assert Y.shape == (N, L, d)
    rc, *got = stats(Y, w)
    want = fields_ref.field_stats(Y, w)
    assert rc == 0
    for what, a, b in zip(("sumse", "sumsc", "sumsd1", "sumsd2"), got, want):
        assert same_bits(a, b), (name, what, np.argwhere(a != b)[:4])
    assert same_bits(got[1], got[1].T) and not np.tril(got[3]).any()
    # without the difference sums, sumse and sumsc keep their bits
    rc2, se, sc, d1, d2 = stats(Y, w, differences=False)
    assert rc2 == 0 and d1 is None and d2 is None and same_bits(se, got[0]) and same_bits(sc, got[1])


def test_host_device_and_slab_boundaries_give_the_same_bits():
    import torch
    from bluest_amd import _lib, fields
    Y, w = real_data(3 * CHUNK + 5, 9, 21, 5)
    rc, *host = stats(Y, w)
    T = torch.from_numpy(Y).cuda()
    torch.cuda.synchronize()
    rc2, *dev = stats(T, w)
    assert rc == 0 and rc2 == 0 and all(same_bits(a, b) for a, b in zip(host, dev))
    lib, before = _lib.lib(), ctypes.c_int64(0)
    assert lib.bluest_group_sums_slab(1, ctypes.byref(before)) == 0
    try:
        rc3, *tiny = stats(Y, w)                                        # one chunk per slab: 4 slabs
        assert lib.bluest_group_sums_slab(2 * CHUNK * 9 * 21 * 8 + 100, None) == 0
        rc4, *mid = stats(Y, w)                                         # two chunks per slab, the last slab short
    finally:
        assert lib.bluest_group_sums_slab(before.value, None) == 0
    assert rc3 == 0 and rc4 == 0 and all(same_bits(a, b) for a, b in zip(host, tiny)) and all(same_bits(a, b) for a, b in zip(host, mid))
    rc5, *again = stats(Y, w)
    assert rc5 == 0 and all(same_bits(a, b) for a, b in zip(host, again))
    # the Python entry: the same sums, sumsd1 spread over [L, L, d]
    for v in (Y, T):
        se, sc, d1, d2 = fields.field_statistics(v, w)
        iu = fields_ref.pairs(9)
        assert same_bits(se, host[0]) and same_bits(sc, host[1]) and same_bits(d2, host[3])
        assert same_bits(d1[iu[0], iu[1]], host[2]) and not d1[np.tril_indices(9)].any()
    se, sc, d1, d2 = fields.field_statistics(Y, w, differences=False)
    assert d1 is None and d2 is None and same_bits(se, host[0]) and same_bits(sc, host[1])


def test_nan_propagates_to_what_it_enters_only():
    Y, w = real_data(CHUNK + 3, 6, 11, 6)
    w[4] = 2.0
    Y[CHUNK + 1, 2, 4] = np.nan
    rc, se, sc, d1, d2 = stats(Y, w)
    assert rc == 0
    hit = np.zeros((6, 11), dtype=bool)
    hit[2, 4] = True
    assert np.array_equal(np.isnan(se), hit)
    with_2 = np.zeros((6, 6), dtype=bool)
    with_2[2, :] = with_2[:, 2] = True
    assert np.array_equal(np.isnan(sc), with_2)
    assert np.array_equal(np.isnan(d2), np.triu(with_2, 1))
    iu = fields_ref.pairs(6)
    assert np.array_equal(np.isnan(d1), ((iu[0] == 2) | (iu[1] == 2))[:, None] & (np.arange(11) == 4)[None, :])


@pytest.mark.parametrize("N,L,d", [(517, 64, 12), (300, 7, 100), (2000, 3, 5)])
def test_real_data_within_the_rounding_bounds(N, L, d):
    """a sum of n terms, each with at most k roundings of its own, is off by at most (n + k) u sum|terms| to first order, in any
    order: n = N for sumse and sumsd1 (k = 0, 1), n = N d for sumsc (k = 2: w a, the fma) and sumsd2 (k = 4: a - b twice more)"""
    Y, w = real_data(N, L, d, N + L + d)
    rc, se, sc, flat, d2 = stats(Y, w)
    assert rc == 0
    iu = fields_ref.pairs(L)
    d1 = np.zeros((L, L, d))
    d1[iu[0], iu[1]] = flat
    (le, lc, l1, l2), (ae, ac, a1, a2) = fields_ref.stats_ld(Y, w)
    worst = {}
    for name, got, ref, bound in (("sumse", se, le, (N + 2) * U * ae), ("sumsc", sc, lc, (N * d + 4) * U * ac),
                                  ("sumsd1", d1, l1, (N + 3) * U * a1), ("sumsd2", d2, l2, (N * d + 6) * U * a2)):
        err, bound = np.abs(got.astype(fields_ref.LD) - ref).astype(np.float64), np.asarray(bound, dtype=np.float64)
        worst[name] = float((err[bound > 0] / bound[bound > 0]).max())
        assert (err <= bound).all(), (name, worst[name])
    print("largest error / bound:", worst)
    # why the difference sums exist: two models 1e-6 apart, from the explicit differences and from C_00 + C_11 - 2 C_01
    inner = lambda a, b: float(np.dot(a * w, b))
    exact = float(l2[0, 1] / N - (l1[0, 1] / N * w * l1[0, 1] / N).sum())
    direct = d2[0, 1] / N - inner(d1[0, 1] / N, d1[0, 1] / N)
    C = lambda i, j: sc[i, j] / N - inner(se[i], se[j]) / N**2
    route = C(0, 0) + C(1, 1) - 2 * C(0, 1)
    print("dV %.17g: explicit differences off by %.2e, covariance route off by %.2e" % (exact, abs(direct / exact - 1), abs(route / exact - 1)))
    assert abs(direct / exact - 1) <= 1e-12
    assert abs(route / exact - 1) > 1e-6


def test_argument_errors():
    from bluest_amd import _lib
    lib = _lib.lib()
    Y, w = np.ones((4, 3, 2)), np.array([1.0, 2.0])
    rc, se, sc, d1, d2 = stats(Y, w)
    assert rc == 0 and (se == 4.0).all() and (sc == 12.0).all() and not d1.any() and not d2.any()
    wide = np.ones(1100000)                                             # 2080 pairs x 1.1e6 components > 2^31 - 1
    bad = {"L = 0": {1: 0}, "L = 65": {1: 65}, "d = 0": {2: 0}, "d < 0": {2: -2}, "N = 0": {0: 0}, "N < 0": {0: -3},
           "values": {3: None}, "w": {4: None}, "sumse": {5: None}, "sumsc": {6: None}, "only sumsd1": {8: None},
           "only sumsd2": {7: None}, "negative weight": {4: np.array([1.0, -1e-300])}, "NaN weight": {4: np.array([np.nan, 1.0])},
           "infinite weight": {4: np.array([1.0, np.inf])}, "too many (pair, component) sums": {1: 64, 2: len(wide), 4: wide},
           "too many (chunk, block of tiles) workgroups": {0: 1 << 45}}
    for what, change in bad.items():
        rc, *out = stats(Y, w, override=change)
        assert rc == ERR_ARG, what
        assert len(lib.bluest_last_error()) > 0, what
        assert all((o == -7.0).all() for o in out), what                # a refused call writes nothing

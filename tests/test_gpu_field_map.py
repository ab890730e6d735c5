"""GPU tests of bluest_field_map (include/bluest_hip.h, Part 18) through bluest_amd.field_maps.map_fields and, where the Python
layer would stand in the way, at the ABI itself: bit for bit against the numpy restatement (tests/field_map_ref.py) at the smallest
shapes that reach every edge -- both sides of the block of 8 samples a wavefront keeps (64 for long rows), of the slice of 64 rows
and of the strip of 512 entries, short and long rows in one slice, long rows that share their columns --, the same bits whatever the memory and the staging budget, the anchors the
header states, every refused argument, and the lifetime of a handle.
Most data has exact products (coefficients of 10 bits, values of 16): the restatement then runs vectorised and p + a * b has fma's
one rounding, while the SUMS round at every step (magnitudes over 40 binary orders); one case walks the exact fma on general data."""
import ctypes

import numpy as np
import pytest

import field_map_ref as ref
from bluest_amd import _lib
from bluest_amd.field_maps import FieldOperator, map_fields
from field_map_ref import same_bits

pytestmark = pytest.mark.gpu

SB = 8                                                                  # samples per wavefront (csrc/field_map.hip)
LENGTHS = [0, 1, 2, 511, 512, 513, 1100, 3]                             # cycled over the rows: short and long rows in every slice
ERR_ARG = 1


def operator(csr):
    return FieldOperator(csr[:3], shape=csr[3])


def cuda(v):
    import torch
    return torch.tensor(v, dtype=torch.float64, device="cuda")


def host(t):
    return t.cpu().numpy() if hasattr(t, "data_ptr") else t


def group(seed, N, q, ds, lengths, identity=()):
    """(values, csr tuples or None, FieldOperators or None) of len(ds) models; the models in `identity` have d = q and no operator"""
    rng = np.random.RandomState(seed)
    csr = [None if l in identity else ref.random_operator(rng, q, d, lengths[l % len(lengths):] + lengths[:l % len(lengths)])
           for l, d in enumerate(ds)]
    values = [ref.data26(rng, N, q if l in identity else d) for l, d in enumerate(ds)]
    return values, csr, [None if c is None else operator(c) for c in csr]


@pytest.fixture(scope="module")
def edges():
    """one operator with every row length of the issue in every slice: q = 130 rows over d = 1100 columns, 19 samples"""
    values, csr, ops = group(1, 19, 130, [1100], LENGTHS)
    return values[0], csr[0], ops[0], ref.apply(csr[0], values[0], exact_products=True)


# ---- bit for bit against the restatement ---------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [1, 2, SB - 1, SB, SB + 1, 2 * SB + 1, 19])
def test_both_sides_of_the_sample_block(edges, N):
    y, csr, op, want = edges
    assert sorted(set(np.diff(csr[0]).tolist())) == sorted(LENGTHS)
    for values in (y[:N], cuda(y[:N])):
        got = host(map_fields([values], [op]))
        assert got.shape == (N, 1, 130) and same_bits(got[:, 0], want[:N])


@pytest.mark.parametrize("d", [1, 7, 64, 1100])
@pytest.mark.parametrize("q", [1, 63, 64, 65, 130])
def test_both_sides_of_the_row_slice(q, d):
    lengths = [0, 1, 2, 513, 5, 1, 600] if d == 1100 else [0, 1, 2, 5, 513 if d == 64 else 3]
    values, csr, ops = group(100 * q + d, 9, q, [d], lengths)
    want = ref.map_fields(values, csr, exact_products=True)
    assert same_bits(host(map_fields(values, ops)), want) and same_bits(host(map_fields([cuda(values[0])], ops)), want)


@pytest.mark.parametrize("L", [1, 2, 3, 17, 64])
def test_models_of_different_widths_with_identity_entries(L):
    q = 65
    ds = [(1, 7, 64, 1100, 33)[l % 5] for l in range(L)]
    identity = set(range(1, L, 3))
    values, csr, ops = group(L, 3, q, ds, [0, 2, 1, 7, 513, 1, 3, 2, 1, 1, 4], identity)
    want = ref.map_fields(values, csr, exact_products=True)
    mixed = [cuda(v) if l % 2 else v for l, v in enumerate(values)]
    got = map_fields(mixed, ops)
    assert (L == 1 or got.is_cuda) and tuple(got.shape) == (3, L, q) and same_bits(host(got), want)
    for l in identity:
        assert same_bits(host(got)[:, l], values[l])


def test_general_data_through_the_exact_fma():
    rng = np.random.RandomState(5)
    csr = ref.random_operator(rng, 6, 9, [0, 1, 2, 9, 600, 3])
    csr = (csr[0], csr[1], rng.randn(len(csr[2])) * 10.0 ** rng.randint(-3, 4, size=len(csr[2])), csr[3])
    y = rng.randn(2, 9) * 10.0 ** rng.randint(-3, 4, size=(2, 9))
    want = ref.apply(csr, y)
    assert same_bits(host(map_fields([y], [operator(csr)]))[:, 0], want)
    print("largest error / bound against the long-double product:", ref.self_check(csr, y))


def test_a_repeated_column_and_the_stored_order_of_a_row():
    """rows 0 and 1 hold the same entries, row 0 with its columns ascending, row 1 as (0, 2, 1): 2^53 + 1 - 2^53 is 0 in the
    first order and 1 in the second; row 2 names column 1 three times"""
    y = np.array([[2.0 ** 53, 1.0, -2.0 ** 53], [3.0, 5.0, 7.0]])
    csr = (np.array([0, 3, 6, 9]), np.array([0, 1, 2, 0, 2, 1, 1, 1, 1]), np.array([1.0] * 6 + [0.5, 0.25, 2.0]), (3, 3))
    want = ref.apply(csr, y, exact_products=True)
    assert want[0, 0] == 0.0 and want[0, 1] == 1.0                      # this data tells the two orders apart
    assert np.array_equal(want[:, 2], 2.75 * y[:, 1])
    assert same_bits(host(map_fields([y], [operator(csr)]))[:, 0], want)
    assert same_bits(host(map_fields([cuda(y)], [operator(csr)]))[:, 0], want)


def test_dense_rows_that_share_their_columns():
    """19 rows over all of 600 columns in ascending order, a row with its columns reversed among them, and short rows: the long-row
    kernel gathers the values once per bundle of up to 8 rows with one column sequence; 70 and 130 samples cross its blocks of 64"""
    rng = np.random.RandomState(17)
    cols = [np.arange(600)] * 5 + [np.arange(600)[::-1], np.arange(3)] + [np.arange(600)] * 14 + [np.arange(600)[:513]]
    indptr = np.concatenate([[0], np.cumsum([len(c) for c in cols])])
    idx = np.concatenate(cols)
    data = rng.randint(-1023, 1024, size=len(idx)) * 2.0 ** rng.randint(-6, 7, size=len(idx))
    csr = (indptr, idx, data, (len(cols), 600))
    y = ref.data26(rng, 130, 600)
    want = ref.apply(csr, y, exact_products=True)
    op = operator(csr)
    for N in (1, 63, 64, 65, 70, 130):
        assert same_bits(host(map_fields([cuda(y[:N])], [op]))[:, 0], want[:N])
    assert same_bits(map_fields([y], [op])[:, 0], want)


# ---- the same bits regardless of memory and staging ----------------------------------------------------------------------------------
def abi_map(N, L, q, handles, pointers, out, stream=None):
    H = None if handles is None else ctypes.cast((ctypes.c_void_p * len(handles))(*handles), ctypes.c_void_p)
    P = None if pointers is None else ctypes.cast((ctypes.c_void_p * len(pointers))(*pointers), ctypes.c_void_p)
    return _lib.lib().bluest_field_map(N, L, q, H, P, out, stream)


@pytest.fixture(scope="module")
def trio():
    """three models onto q = 70: a wide operator with long rows, the identity, a narrow operator; 19 samples"""
    values, csr, ops = group(3, 19, 70, [1100, 70, 7], LENGTHS, identity={1})
    return values, ops, ref.map_fields(values, csr, exact_products=True)


def test_host_device_mixed_and_offset_memory_give_the_same_bits(trio):
    import torch
    values, ops, want = trio
    N, L, q = want.shape
    on_gpu = [cuda(v) for v in values]
    assert same_bits(map_fields(values, ops), want)
    for vals in (on_gpu, [values[0], on_gpu[1], values[2]], [on_gpu[0], values[1], on_gpu[2]]):
        got = map_fields(vals, ops)
        assert got.is_cuda and same_bits(host(got), want)
    # a base offset by 8 bytes, on either side, and `out` on the side the values are not on
    shifted = []
    for v in values:
        buf = np.zeros(v.size + 1)
        buf[1:] = v.reshape(-1)
        shifted.append(buf[1:].reshape(v.shape))
        assert shifted[-1].ctypes.data == buf.ctypes.data + 8
    dev_shifted = [cuda(np.concatenate([[0.0], v.reshape(-1)]))[1:].view(v.shape) for v in values]
    handles = [None if op is None else op.handle() for op in ops]
    for vals in (shifted, dev_shifted):
        for out in (np.full(N * L * q + 1, -7.0), torch.full((N * L * q + 1,), -7.0, dtype=torch.float64, device="cuda")):
            torch.cuda.synchronize()
            assert abi_map(N, L, q, handles, [_lib.ptr(v) for v in vals], _lib.ptr(out[1:])) == 0
            assert same_bits(host(out)[1:].reshape(N, L, q), want) and host(out)[0] == -7.0


def test_the_staging_budget_never_shows(trio):
    values, ops, want = trio
    for slab_bytes in (1, 3 * 8 * (1100 + 70 + 7 + 3 * 70) + 5, 1 << 30):           # a sample per run, three, all of them
        assert same_bits(map_fields(values, ops, slab_bytes=slab_bytes), want)
        assert same_bits(host(map_fields([cuda(values[0]), values[1], values[2]], ops, slab_bytes=slab_bytes)), want)


def test_a_model_alone_and_as_one_of_seventeen(trio):
    values, ops, want = trio
    alone = map_fields(values[:1], ops[:1])
    many = map_fields([values[l % 3] for l in range(17)], [ops[l % 3] for l in range(17)])
    assert same_bits(alone[:, 0], want[:, 0])
    for l in range(17):
        assert same_bits(many[:, l], want[:, l % 3])


# ---- the anchors of the header -------------------------------------------------------------------------------------------------------
def test_identity_copies_bits():
    y = np.array([[-0.0, 1.5, np.nan], [np.inf, -np.inf, 5e-324]])
    y.view(np.uint64)[0, 2] = 0x7ff800000000beef                        # a NaN with a payload
    for vals in ([y], [cuda(y)]):
        assert same_bits(host(map_fields(vals, [None]))[:, 0], y)
    both = map_fields([y, y[:, :2]], [None, operator((np.array([0, 0, 1, 1]), np.array([1]), np.array([1.0]), (3, 2)))])
    assert same_bits(both[:, 0], y) and same_bits(both[:, 1], np.array([[0.0, 1.5, 0.0], [0.0, -np.inf, 0.0]]))


def test_an_empty_row_gives_plus_zero():
    csr = (np.array([0, 0, 1, 1]), np.array([0]), np.array([-1.0]), (3, 1))
    got = host(map_fields([cuda(np.array([[0.0], [2.0]]))], [operator(csr)]))[:, 0]
    assert same_bits(got, np.array([[0.0, 0.0, 0.0], [0.0, -2.0, 0.0]]))          # (+0.0 also from fma(-1, +0.0, +0.0))


def test_a_zero_coefficient_on_finite_values_leaves_the_chain_alone(edges):
    y, csr, op, want = edges
    indptr, idx, data, shape = csr
    rows = [r for r in range(shape[0]) if indptr[r + 1] - indptr[r] in (2, 511, 513)]
    at = sorted(int(indptr[r]) + 1 for r in rows)                       # a zero as the second entry of these rows
    grown = np.array(indptr)
    for k in at:
        grown[np.searchsorted(indptr, k, side="right"):] += 1
    where = np.array(at) + np.arange(len(at))
    idx2, data2 = np.insert(idx, at, 5), np.insert(data, at, 0.0)
    assert np.all(data2[where] == 0.0) and len(rows) >= 6
    # a row of 511 entries stays one strip with 512; in a row of 513 the extra entry moves every later entry one place on, one of
    # them into the next strip, so only the rows that stay within one strip keep the bits of the operator without the zeros
    one_strip = [r for r in rows if grown[r + 1] - grown[r] <= ref.STRIP]
    got = host(map_fields([y], [operator((grown, idx2, data2, shape))]))[:, 0]
    assert len(one_strip) >= 4 and same_bits(got[:, one_strip], want[:, one_strip])
    assert same_bits(got, ref.apply((grown, idx2, data2, shape), y, exact_products=True))


def test_a_nan_reaches_exactly_the_rows_that_name_its_column(trio):
    values, ops, want = trio
    s, c = 11, 4
    poisoned = [v.copy() for v in values]
    poisoned[0][s, c] = np.nan
    indptr, idx, data = ops[0].csr()
    zero = np.array(data)
    named = np.array([c in idx[indptr[r]:indptr[r + 1]] for r in range(70)])
    zero[idx == c] = 0.0                                                # whatever their coefficient: 0 * NaN is NaN
    assert 2 <= named.sum() < 70 and any(indptr[r + 1] - indptr[r] > ref.STRIP for r in np.flatnonzero(named))
    for op0 in (ops[0], FieldOperator((indptr, idx, zero), shape=ops[0].shape)):
        clean = host(map_fields([cuda(v) for v in values], [op0] + ops[1:]))
        got = host(map_fields([cuda(v) for v in poisoned], [op0] + ops[1:]))
        assert np.array_equal(np.isnan(got[s, 0]), named) and not np.isnan(clean).any()
        got[s, 0, named] = clean[s, 0, named]
        assert same_bits(got, clean)                                    # no other sample, model or row


# ---- errors and lifetime -------------------------------------------------------------------------------------------------------------
def test_every_refused_operator():
    lib = _lib.lib()

    def create(q, d, indptr, indices, data, with_handle=True):
        h = ctypes.c_void_p()
        arrays = [None if a is None else np.ascontiguousarray(a, dtype=t) for a, t in zip((indptr, indices, data), (np.int64, np.int32, np.float64))]
        rc = lib.bluest_field_op_create(q, d, *[_lib.ptr(a) for a in arrays], ctypes.byref(h) if with_handle else None)
        assert h.value is None or rc == 0
        return rc, h
    good = ([0, 1, 2], [0, 1], [1.0, 2.0])
    rc, h = create(2, 2, *good)
    shape = [ctypes.c_int64() for _ in range(3)]
    assert rc == 0 and lib.bluest_field_op_shape(h, *[ctypes.byref(x) for x in shape]) == 0 and [x.value for x in shape] == [2, 2, 2]
    assert lib.bluest_field_op_destroy(h) == 0
    assert lib.bluest_field_op_destroy(None) == ERR_ARG and lib.bluest_field_op_shape(None, None, None, None) == ERR_ARG
    bad = {
        "q < 1": (0, 2, [0], [], []), "d < 1": (2, 0) + good, "d above 2^31 - 1": (2, 2**31) + good, "q above 2^31 - 1": (2**31, 2, [0], [], []),
        "nnz above 2^31 - 1": (1, 2, [0, 2**31], [0], [1.0]), "indptr[0] != 0": (2, 2, [1, 1, 2], [0, 1], [1.0, 2.0]),
        "indptr decreasing": (2, 2, [0, 2, 1], [0, 1], [1.0, 2.0]), "an index of d": (2, 2, [0, 1, 2], [0, 2], [1.0, 2.0]),
        "a negative index": (2, 2, [0, 1, 2], [-1, 1], [1.0, 2.0]), "an infinite coefficient": (2, 2, [0, 1, 2], [0, 1], [1.0, np.inf]),
        "a NaN coefficient": (2, 2, [0, 1, 2], [0, 1], [np.nan, 1.0]), "a null indptr": (2, 2, None, [0, 1], [1.0, 2.0]),
        "a null indices": (2, 2, [0, 1, 2], None, [1.0, 2.0]), "a null data": (2, 2, [0, 1, 2], [0, 1], None),
    }
    for why, args in bad.items():
        assert create(*args)[0] == ERR_ARG, why
        assert b"" != lib.bluest_last_error()
    assert create(2, 2, *good, with_handle=False)[0] == ERR_ARG


def test_every_refused_call_leaves_out_untouched():
    import torch
    q, d, N = 3, 2, 4
    op, other = operator(ref.random_operator(np.random.RandomState(0), q, d, [1, 2])), operator(ref.random_operator(np.random.RandomState(0), q + 1, d, [1]))
    y, z = cuda(np.ones((N + 1, d))), cuda(np.ones((N + 1, q)))
    out = torch.full((N * 65 * q + 1,), -7.0, dtype=torch.float64, device="cuda")
    h, yp, zp, op_ = op.handle(), y.data_ptr(), z.data_ptr(), out.data_ptr()
    bad = {
        "L = 0": (N, 0, q, [h], [yp], op_), "L = 65": (N, 65, q, [h] * 65, [yp] * 65, op_), "N < 0": (-1, 1, q, [h], [yp], op_),
        "q < 1": (N, 1, 0, [h], [yp], op_), "another q": (N, 2, q, [h, other.handle()], [yp, yp], op_), "the call's q": (N, 1, q + 1, [h], [yp], op_),
        "null values": (N, 1, q, [h], None, op_), "a null values[l]": (N, 2, q, [h, None], [yp, None], op_), "a null out": (N, 1, q, [h], [yp], None),
        "values[l] off by 4 bytes": (N, 2, q, [None, h], [zp, yp + 4], op_), "out off by 4 bytes": (N, 1, q, [h], [yp], op_ + 4),
    }
    for why, args in bad.items():
        assert abi_map(*args) == ERR_ARG, why
    torch.cuda.synchronize()
    assert bool((out == -7.0).all())
    with pytest.raises(_lib.BluestHipError):
        map_fields([np.ones((N, d))] * 65, [op] * 65)
    # N == 0: nothing is written, an empty result comes back; a null list of operators is all identity
    assert abi_map(0, 1, q, [h], [None], None) == 0 and abi_map(N, 1, q, None, [zp], op_ + 8) == 0
    torch.cuda.synchronize()
    assert bool((out[1:1 + N * q] == 1.0).all()) and out[0] == -7.0 and bool((out[1 + N * q:] == -7.0).all())
    empty = map_fields([np.zeros((0, d)), cuda(np.zeros((0, q)))], [op, None])
    assert empty.is_cuda and tuple(empty.shape) == (0, 2, q)
    assert map_fields([np.zeros((0, d))], [op]).shape == (0, 1, q)


def test_a_hundred_handles_come_and_go():
    rng = np.random.RandomState(9)
    y = ref.data26(rng, 3, 5)
    dev = cuda(y)
    for i in range(100):
        csr = ref.random_operator(rng, 1 + i % 4, 5, [2, 0, 3])
        op = operator(csr)
        got = map_fields([dev if i % 2 else y], [op])
        assert op._handle is not None and same_bits(host(got)[:, 0], ref.apply(csr, y, exact_products=True))
        del op

"""
Host tests of bluest_amd.field_stream (include/bluest_hip.h, Part 19): the numpy restatement of the streamed order
(tests/field_accum_ref.py) has the bits of the one-shot restatements on the concatenation, for every way of cutting a segment into
updates -- the equality argument, checked without a GPU; the symbols are declared, exported and bound; arguments are refused
before any device call; and StreamedFieldsMixin, with the restatements standing in for the kernels, makes the sampler calls of its
unstreamed twin and returns its bits from solve(), the sampled errors, field_sample_moments and variance_test, with flushes
inside the repeats and with mapped fields too.  tests/test_gpu_field_stream.py runs the same problem on the real kernels.
"""
import ctypes
import os
import weakref

import numpy as np
import pytest

import field_accum_ref as aref
import field_map_ref
import field_moments_ref as mref
import fields_ref
from gsums_ref import same_bits

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
SYMBOLS = ["bluest_field_accum_create", "bluest_field_accum_update", "bluest_field_accum_finish", "bluest_field_accum_info",
           "bluest_field_accum_destroy"]

M, D = 3, 5
MASS = np.array([0.5, 1.0, 2.0, 0.25, 1.5])
AMP = np.array([1.0, -0.5, 2.0, 0.1, 0.7])
GROUPS = [[0, 1, 2], [0, 1], [1, 2], [2], [0, 2], [1]]
SAMPLES = np.array([9, 0, 140, 300, 1, 5])                              # group 1 is not drawn, group 4 once; 140 and 300 cross chunks
BATCH = 50                                                              # never aligned with the chunks of 128


def splits(N):
    """the ways a segment of N rows is cut into updates: all at once, row by row (small N), the list of the GPU test"""
    out = [[N]]
    if N <= 130:
        out.append([1] * N)
    mixed, left = [], N
    for n in [1, 126, 1, 128, 300, 0, 127]:
        mixed.append(min(n, left))
        left -= mixed[-1]
    out.append(mixed + [left])
    return out


def streamed(values, coef, sizes, exact=False):
    acc = aref.FieldAccumRef(values.shape[1], values.shape[2], coef, exact_products=exact)
    at = 0
    for n in sizes:
        acc.update(values[at:at + n])
        at += n
    assert at == values.shape[0]
    return acc.finish()


# ---- (a) the equality argument --------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("N", [0, 1, 127, 128, 129, 300, 700])
def test_the_streamed_order_has_the_bits_of_the_one_shot_order(N):
    L, d = 3, 2
    v, coef = mref.data26(N, L, d, seed=N + 1, signed=True)
    want_s = fields_ref.segment_sums(v)
    want_z = mref.segment_moments(v, coef, exact_products=True)
    for sizes in splits(N):
        count, sums, zsum, zsq = streamed(v, coef, sizes, exact=True)
        assert count == N and same_bits(sums, want_s) and same_bits(zsum, want_z[0]) and same_bits(zsq, want_z[1]), sizes
        count, sums, zsum, zsq = streamed(v, None, sizes)
        assert count == N and same_bits(sums, want_s) and zsum is None and zsq is None
    if N <= 1:
        assert not np.signbit(want_z[0]).any() and (want_z[0] == 0).all() and (want_z[1] == 0).all()


def test_the_exact_fma_gives_the_same_agreement_on_ordinary_data():
    rng = np.random.RandomState(4)
    v, coef = 1.5 + rng.randn(300, 2, 3), rng.randn(2)
    want_s, want_z = fields_ref.segment_sums(v), mref.segment_moments(v, coef)
    for sizes in ([300], [50] * 6, [1, 126, 1, 128, 44]):
        count, sums, zsum, zsq = streamed(v, coef, sizes)
        assert count == 300 and same_bits(sums, want_s) and same_bits(zsum, want_z[0]) and same_bits(zsq, want_z[1])


def test_lanes_take_a_second_chunk_across_updates():
    """8357 rows = 65 chunks + 37: lanes 0 and 1 add a second chunk, in another update than their first, and a tail remains"""
    N = 65 * 128 + 37
    v, coef = mref.data26(N, 2, 1, seed=9)
    want_s, want_z = fields_ref.segment_sums(v), mref.segment_moments(v, coef, exact_products=True)
    for sizes in ([N], [500] * 16 + [357], [8191, 1, 128, 37], [64 * 128, 165]):
        acc = aref.FieldAccumRef(2, 1, coef, exact_products=True)
        at = 0
        for n in sizes:
            acc.update(v[at:at + n])
            at += n
        assert acc.tail.shape[0] == 37 and acc.chunks_done == 65
        count, sums, zsum, zsq = acc.finish()
        assert acc.chunks_done == 66 and count == N
        assert same_bits(sums, want_s) and same_bits(zsum, want_z[0]) and same_bits(zsq, want_z[1]), sizes


def test_a_sum_fed_back_as_one_sample_keeps_its_bits():
    """what StreamedFieldsMixin relies on at a flush: [1, L, d] passes through the one-shot order unchanged"""
    rng = np.random.RandomState(2)
    s = rng.randn(3, 5) * 10.0 ** rng.uniform(-8, 8, (3, 5))
    s[1, 2] = 0.0
    assert same_bits(fields_ref.segment_sums(s[None]), s)


# ---- (b) the build and the binding -----------------------------------------------------------------------------------------------
def test_the_symbols_are_declared_exported_and_bound():
    from bluest_amd import _lib, build
    assert "field_accum.hip" in build.SOURCES and "field_partials.hpp" in build.HEADERS
    header = open(os.path.join(ROOT, "include", "bluest_hip.h")).read()
    build.build()
    so = ctypes.CDLL(_lib.LIB_PATH)
    for name in SYMBOLS:
        assert ("int %s(" % name) in header and hasattr(so, name) and name in _lib.SIGNATURES
        assert getattr(_lib.lib(), name).argtypes == _lib.SIGNATURES[name]
    assert "Part 19" in header
    assert [len(_lib.SIGNATURES[n]) for n in SYMBOLS] == [5, 4, 6, 2, 1]
    assert _lib.lib().bluest_abi_version() == 1


# ---- (c) arguments are refused before any device call ---------------------------------------------------------------------------
def test_the_c_entry_points_check_their_arguments_first():
    import torch
    from bluest_amd import _lib
    lib = _lib.lib()
    h = ctypes.c_void_p()
    ok, nan = np.ones(3), np.array([1.0, np.nan, 1.0])
    create = lambda L, d, coef, out=h: lib.bluest_field_accum_create(L, d, _lib.ptr(coef), ctypes.byref(out) if out is not None else None, None)
    assert create(0, 5, None) == 1 and create(65, 5, None) == 1 and create(3, 0, None) == 1 and create(3, 5, nan) == 1
    assert lib.bluest_field_accum_create(3, 5, None, None, None) == 1 and h.value is None
    v = np.ones((4, 3, 5))
    count = ctypes.c_int64(-7)
    sums = np.full((3, 5), -7.0)
    assert lib.bluest_field_accum_update(None, 4, _lib.ptr(v), None) == 1
    assert lib.bluest_field_accum_finish(None, ctypes.byref(count), _lib.ptr(sums), None, None, None) == 1
    assert lib.bluest_field_accum_info(None, None) == 1 and lib.bluest_field_accum_destroy(None) == 0
    assert count.value == -7 and (sums == -7.0).all()
    if not torch.cuda.is_available():
        assert create(3, 5, ok) == 3 and h.value is None                # BLUEST_ERR_NOGPU: there is no CPU path


def test_the_accumulator_checks_its_arguments_before_it_touches_the_device(monkeypatch):
    import torch
    from bluest_amd import _lib, field_stream
    called = []
    real = _lib.lib
    monkeypatch.setattr(_lib, "lib", lambda: called.append(1) or real())
    for L, d, coef in [(0, 5, None), (65, 5, None), (3, 0, None), (3, 5, np.ones(2)), (3, 5, np.array([1.0, np.inf, 0.0]))]:
        with pytest.raises(ValueError):
            field_stream.FieldAccumulator(L, d, coef)
    acc = field_stream.FieldAccumulator(3, 5, np.ones(3))
    for bad in (np.ones((4, 2, 5)), np.ones((4, 3, 4)), np.ones((4, 15)), torch.ones(4, 3, 5, dtype=torch.float32)):
        with pytest.raises(ValueError):
            acc.update(bad)
    acc.close()
    with pytest.raises(ValueError):
        acc.update(np.ones((4, 3, 5)))                                  # closed
    assert not called
    with pytest.raises(ValueError):
        type("P", (field_stream.StreamedFieldsMixin, object), {})(field_stream_bytes=-1)


# ---- the problem of (d) -----------------------------------------------------------------------------------------------------------
def _bases(*front):
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.field_errors import FieldErrorsMixin
    from bluest_amd.fields import FieldOutputsMixin
    return tuple(front) + (FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem)


def model_covariances():
    A = np.array([[1.0, 0.6, 0.3], [0.6, 1.2, 0.5], [0.3, 0.5, 0.9]])
    return [A, float(np.dot(AMP * MASS, AMP)) * A]


def toy(bases, seed=3, poison=(3,), cuda=False, operators=None, **kw):
    """one number and one field of D components per model, in batches of BATCH; evaluate call number `poison` returns a NaN, so
    that batch is drawn again.  With `operators` models 1 and 2 return their field on meshes of 3 and 2 points."""
    native = {0: D, 1: 3, 2: 2} if operators is not None else {0: D, 1: D, 2: D}

    class Toy(*bases):
        def output_weights(self): return [None, MASS]

        def output_operators(self): return operators if operators is not None else [None, None]

        def sampler(self, ls, N=1):
            self.calls.append((list(ls), int(N)))
            z = self.rng.randn(int(N), 1 + len(ls))
            return [(z[:, 0], z[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples, N=1):
            self.evaluations += 1
            y = [2.0 + 0.8 ** l * s[0] + 0.3 * (l + 1) * s[1] for l, s in zip(ls, samples)]
            field = [AMP[None, :native[l]] * v[:, None] + np.arange(native[l])[None, :] for l, v in zip(ls, y)]
            if self.evaluations in poison:
                field[-1][0, 0] = np.nan
            if cuda:
                import torch
                return [[torch.from_numpy(v).cuda() for v in y], [torch.from_numpy(f).cuda() for f in field]]
            return [y, field]

    args = dict(C=model_covariances(), costs=np.array([4.0, 2.0, 1.0]), n_outputs=2, verbose=False, sample_batch_size=BATCH)
    args.update(kw)
    p = Toy(M, **args)
    p.rng, p.calls, p.evaluations = np.random.RandomState(seed), [], 0
    return p


def hand_set(p, seed=5):
    """the allocation in place of setup_solver, and random weights in place of the GPU solve; output 1 does not see group 5"""
    chosen = np.flatnonzero(SAMPLES > 0)
    T = sum(len(GROUPS[g]) for g in chosen)
    W = np.random.RandomState(seed).randn(2, T)
    W[1, T - 1:] = 0.0
    Vs = np.array([0.04, 0.09])
    out = {"budget": None, "eps": [0.2, 0.3], "samples": SAMPLES, "flattened_groups": GROUPS, "variances": Vs, "cost": 7.0}
    p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (W, Vs))
    return W


def everything(p):
    """what a user reads off a problem after solve(): the twins must agree on every bit of it"""
    mus, errs, cost = p.solve(K=3, eps=[0.2, 0.3])
    got = {"mus0": np.array([mus[0]]), "mus1": mus[1], "errs": errs, "cost": np.array([cost]), "sampled": p.sampled_errors()}
    maps, unsampled = p.sampled_error_fields()
    got["map0"], got["map1"], got["unsampled"] = np.array([maps[0]]), maps[1], np.array(unsampled)
    for n, per_group in enumerate(p.field_sample_moments):
        for g, (N, var) in per_group.items():
            got["var_%d_%d" % (n, g)] = np.concatenate([[float(N)], var])
    got["n_moments"] = np.array([float(len(m)) for m in p.field_sample_moments])
    ex, err = p.variance_test(eps=[0.2, 0.3], K=3, N=3)
    got["vt_ex"], got["vt"] = ex, err
    return got, list(p.calls)


def assert_twins(a, b):
    (got_a, calls_a), (got_b, calls_b) = a, b
    assert calls_a == calls_b and sorted(got_a) == sorted(got_b)
    for key in got_a:
        assert same_bits(got_a[key], got_b[key]), key


@pytest.fixture
def stubbed(monkeypatch):
    """the one-shot calls and the accumulator -> their restatements"""
    from bluest_amd import field_errors, field_maps, field_stream, fields
    monkeypatch.setattr(fields, "field_group_sums", lambda values, **kw: fields_ref.field_group_sums(values, **kw))
    monkeypatch.setattr(field_errors, "field_weighted_moments", lambda values, coef, **kw: mref.field_weighted_moments(values, coef))
    monkeypatch.setattr(field_maps, "map_fields", lambda values, operators, **kw: field_map_ref.map_fields(values, operators))
    monkeypatch.setattr(field_stream, "FieldAccumulator", aref.StubAccumulator)
    del aref.StubAccumulator.made[:]
    return aref.StubAccumulator.made


def test_the_streamed_problem_is_its_unstreamed_twin(stubbed):
    from bluest_amd.field_stream import StreamedFieldsMixin
    plain = toy(_bases())
    hand_set(plain)
    want = everything(plain)
    assert not stubbed
    assert len(plain.calls) == 4 * (sum(-(-int(m) // BATCH) for m in SAMPLES)) + 1      # solve, three repeats, one batch drawn again
    p = toy(_bases(StreamedFieldsMixin), field_stream_bytes=0)
    hand_set(p)
    got = everything(p)
    assert_twins(got, want)
    chosen = np.flatnonzero(SAMPLES > 0)
    assert len(stubbed) == 4 * 2 * len(chosen) and all(a.closed for a in stubbed)        # an accumulator per group, output and repeat
    by_group = [a.updates for a in stubbed[:2 * len(chosen):2]]
    assert by_group == [[9], [50, 50, 40], [50] * 6, [1], [5]]                          # batch by batch, never joined
    assert all(a.ref.coef is not None for a in stubbed[:2 * len(chosen)])               # solve() collects: the group's BLUE weights
    assert all(a.ref.coef is None for a in stubbed[2 * len(chosen):])                   # a variance test's repeats are not looked at
    # below the threshold the mix-in is its bases: the default keeps this small problem unstreamed
    del stubbed[:]
    q = toy(_bases(StreamedFieldsMixin))
    hand_set(q)
    assert q.field_stream_bytes == 256 << 20
    assert_twins(everything(q), want)
    assert not stubbed
    # a threshold in between streams the large groups only: 300 * 1 * 6 * 8 = 14400 and 140 * 2 * 6 * 8 = 13440
    h = toy(_bases(StreamedFieldsMixin), field_stream_bytes=13440)
    hand_set(h)
    assert_twins(everything(h), want)
    assert len(stubbed) == 4 * 2 * 2 and sorted(set(a.ref.L for a in stubbed)) == [1, 2]


def test_flushes_inside_the_repeats_and_mapped_fields(stubbed, monkeypatch):
    from bluest_amd import fields
    from bluest_amd.field_maps import MappedFieldsMixin
    from bluest_amd.field_stream import StreamedFieldsMixin
    whole = toy(_bases())
    hand_set(whole)
    want_whole = everything(whole)
    monkeypatch.setattr(fields, "SLAB_BYTES", 1)                        # a flush after every group
    plain = toy(_bases())
    hand_set(plain)
    want = everything(plain)
    p = toy(_bases(StreamedFieldsMixin), field_stream_bytes=0)
    hand_set(p)
    assert_twins(everything(p), want)
    for key in ("var_1_3", "var_0_2", "sampled"):
        assert same_bits(want[0][key], want_whole[0][key])              # (where a flush falls never shows in the moments)
    h = toy(_bases(StreamedFieldsMixin), field_stream_bytes=13440)      # held and streamed segments in turn
    hand_set(h)
    assert_twins(everything(h), want)
    monkeypatch.setattr(fields, "SLAB_BYTES", 20000)                    # flushes that hold a held and a streamed group together
    P1, P2 = field_map_ref.interpolation_1d(3, D), field_map_ref.interpolation_1d(2, D)
    operators = [None, [None, (P1[:3], P1[3]), (P2[:3], P2[3])]]
    mapped = toy(_bases(MappedFieldsMixin), operators=operators)
    hand_set(mapped)
    want_mapped = everything(mapped)
    assert not same_bits(want_mapped[0]["mus1"], want[0]["mus1"])
    for threshold in (0, 13440):
        m = toy(_bases(StreamedFieldsMixin, MappedFieldsMixin), operators=operators, field_stream_bytes=threshold)
        hand_set(m)
        assert_twins(everything(m), want_mapped)


def test_group_sums_of_the_other_estimators_are_streamed_too(stubbed):
    """_group_sums is the path of MFMC, MLMC, MC and BLUEProblem.solve"""
    from bluest_amd.field_stream import StreamedFieldsMixin
    plain, p = toy(_bases(), poison=(2,)), toy(_bases(StreamedFieldsMixin), poison=(2,), field_stream_bytes=0)
    want = plain._group_sums([0, 2], 333)
    got = p._group_sums([0, 2], 333)
    assert p.calls == plain.calls and len(p.calls) == 8
    assert len(stubbed) == 2 and stubbed[0].updates == [50] * 6 + [33] and all(a.ref.coef is None and a.closed for a in stubbed)
    for n in range(2):
        for i in range(2):
            assert type(got[n][i]) is type(want[n][i]) and same_bits(got[n][i], want[n][i])
    empty, want_empty = p._group_sums([0, 2], 0), plain._group_sums([0, 2], 0)
    assert empty[0] == want_empty[0] == [0.0, 0.0] and all(same_bits(a, b) for a, b in zip(empty[1], want_empty[1]))
    assert len(stubbed) == 2                                         # nothing to stream in an empty group


# ---- (e) one batch at a time ----------------------------------------------------------------------------------------------------------
def test_the_generator_hands_out_one_batch_at_a_time():
    from bluest_amd.fields import draw_field_values, field_batches
    p, q = toy(_bases()), toy(_bases())
    seen, shapes = [], []
    for batch in field_batches(p, [0, 1, 2], 170, [1, D]):
        assert all(r() is None for r in seen), "an earlier batch is still alive when the next one arrives"
        shapes.append([b.shape for b in batch])
        seen.extend(weakref.ref(b) for b in batch)
        del batch
    assert shapes == [[(50, 3, 1), (50, 3, D)]] * 3 + [[(20, 3, 1), (20, 3, D)]]
    assert p.calls == [([0, 1, 2], 50)] * 3 + [([0, 1, 2], 50), ([0, 1, 2], 20)]       # the third batch was drawn again
    whole = draw_field_values(q, [0, 1, 2], 170, [1, D])
    assert q.calls == p.calls and whole[1].shape == (170, 3, D)
    again = toy(_bases())
    joined = [np.concatenate(parts) for parts in zip(*field_batches(again, [0, 1, 2], 170, [1, D]))]
    assert same_bits(joined[0], whole[0]) and same_bits(joined[1], whole[1])


# ---- (f) what is refused ----------------------------------------------------------------------------------------------------------------
def test_what_is_refused(stubbed):
    from bluest_amd.field_covariances import FieldCovariancesMixin
    from bluest_amd.field_stream import StreamedFieldsMixin
    from bluest_amd.sap import BLUESTError
    from test_estimator_host import FakeComm
    p = toy(_bases(StreamedFieldsMixin), field_stream_bytes=0, comm=FakeComm(0, 2, {}))
    hand_set(p)
    with pytest.raises(BLUESTError, match="more than one rank"):
        p._sample_estimators(1)
    with pytest.raises(BLUESTError, match="more than one rank"):
        p._group_sums([0, 1], 10)
    c = toy(_bases(StreamedFieldsMixin, FieldCovariancesMixin), field_stream_bytes=0)
    hand_set(c)
    with pytest.raises(BLUESTError, match="FieldCovariancesMixin"):
        c.solve(K=3, eps=[0.2, 0.3])
    assert not p.calls and not c.calls and not stubbed                   # refused before anything is drawn

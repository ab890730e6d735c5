"""
GPU tests of bluest_mlmc_search (csrc/mlmc.hip) at its own interface, called through ctypes as MLMCMixin._mlmc_search calls it,
against the numpy restatement tests/mlmc_ref.py on the case table tests/mlmc_cases.py (whose coverage test_mlmc_ref.py checks on
the CPU).

rc, status, best_mask and best_combo must equal the restatement; best_obj must be bit-equal: both sides evaluate the same
expressions in the same order, each operation correctly rounded, the kernel without contraction.
"""
import ctypes
import struct
import time

import numpy as np
import pytest

import mlmc_cases as mc
import mlmc_ref as ref

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()
UNTOUCHED = 0x5a5a5a5a


def call(args, outputs_given=True, **change):
    """(rc, status, best_mask, best_combo, best_obj, seconds) of one call; `change` replaces arguments"""
    from bluest_amd import _lib
    a = dict(args)
    a.update(change)
    n_out = max(int(args["n_out"]), 1)
    mask, obj, status = ctypes.c_uint32(UNTOUCHED), ctypes.c_double(-7.0), ctypes.c_int32(-7)
    combo = np.full(max(n_out, 64), UNTOUCHED, dtype=np.uint32)
    keep = [None if a[k] is None else np.ascontiguousarray(a[k]) for k in ("eps2", "w", "lv", "adj")]
    t0 = time.perf_counter()
    rc = _lib.lib().bluest_mlmc_search(int(a["nb"]), int(a["n_out"]), int(a["flags"]), float(a["budget"]),
                                       *[_lib.ptr(x) for x in keep],
                                       ctypes.byref(mask), _lib.ptr(combo) if outputs_given else None, ctypes.byref(obj),
                                       ctypes.byref(status), None)
    return rc, status.value, mask.value, combo[:n_out].copy(), obj.value, time.perf_counter() - t0


def bits(x):
    return struct.pack("<d", x)


def check(c, repeat=1):
    r = mc.reference(c)
    assert r.rc == c["rc"]
    first = None
    for _ in range(repeat):
        rc, status, mask, combo, obj, sec = call(c["args"])
        print("%s: rc %d status %d mask %#x obj %r, %.3f s" % (c["name"], rc, status, mask, obj, sec))
        assert rc == r.rc
        assert status == r.status
        if status == ref.TOO_BIG:                                 # nothing else is written
            assert mask == UNTOUCHED and obj == -7.0 and (combo == UNTOUCHED).all()
            continue
        assert mask == r.best_mask
        assert np.array_equal(combo, r.best_combo)
        assert bits(obj) == bits(r.best_obj), (obj, r.best_obj)
        if first is None: first = (status, mask, combo.tolist(), bits(obj))
        assert (status, mask, combo.tolist(), bits(obj)) == first     # a second call on the same inputs: bit-identical


def _ids(*groups):
    return [c["name"] for c in CASES if c["group"] in groups]


def _case(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.fixture(autouse=True, scope="module")
def _library():
    from bluest_amd import build
    build.build()


@pytest.mark.parametrize("name", _ids("base"))
def test_base(name):
    check(_case(name), repeat=2)


@pytest.mark.parametrize("name", _ids("veto_plain", "veto"))
def test_one_output_vetoes(name):
    """a NaN level variance in one output alone removes every group through that pair"""
    check(_case(name))


@pytest.mark.parametrize("name", _ids("graph"))
def test_sparse_graphs(name):
    """nb >= 21: the scan's grid-stride loop over 2^21 and 2^30 masks, paths not cliques, winners with a bit at or above 20"""
    check(_case(name))


@pytest.mark.parametrize("name", _ids("window"))
def test_windows(name):
    """more than CAND_CAP candidates: the host loop bisects its windows and `best` tightens them"""
    check(_case(name))


@pytest.mark.parametrize("name", _ids("tie"))
def test_ties_go_to_the_earlier_group(name):
    """two groups share the best objective bit for bit; five calls give the one answer"""
    check(_case(name), repeat=5)


@pytest.mark.parametrize("name", _ids("status"))
def test_status(name):
    """NONE; TOO_BIG with the outputs untouched; the TOO_BIG input answers in continuous mode"""
    check(_case(name))
    check(mc.valid_small())


@pytest.mark.parametrize("name,change", mc.arg_cases(), ids=[n for n, _ in mc.arg_cases()])
def test_argument_checks(name, change):
    """every bad argument is refused before any launch, with a message, and a valid call still succeeds afterwards"""
    from bluest_amd import _lib
    v = mc.valid_small()
    change = dict(change)
    given = change.pop("outputs_given", True)
    rc, status, mask, combo, obj, _ = call(v["args"], outputs_given=given, **change)
    assert rc == ref.ERR_ARG and _lib.lib().bluest_last_error()
    assert status == -7 and mask == UNTOUCHED and obj == -7.0
    check(v)

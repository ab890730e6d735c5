"""
GPU tests of bluest_mfmc_search (csrc/mfmc.hip) at its own interface, called through ctypes as BLUEProblem._mfmc_search calls
it, against the numpy restatement oracle/mfmc_ref.py on the case table tests/mfmc_cases.py (whose soundness and coverage
test_mfmc_ref.py checks on the CPU).

status, best_mask and best_combo must equal the reference; best_obj must be bit-equal: both sides evaluate the same
expressions in the same order, each operation correctly rounded, the kernel without contraction.
"""
import ctypes
import struct
import time

import numpy as np
import pytest

import mfmc_cases as mc
from oracle import mfmc_ref as ref

pytestmark = pytest.mark.gpu

CASES = mc.all_cases()


def call(args, outputs_given=True, **change):
    """(rc, status, best_mask, best_combo, best_obj, seconds) of one call; `change` replaces arguments"""
    from bluest_amd import _lib
    a = dict(args)
    a.update(change)
    n_out = max(int(args["n_out"]), 1)
    mask, obj, status = ctypes.c_uint32(0x5a5a5a5a), ctypes.c_double(-7.0), ctypes.c_int32(-7)
    combo = np.full(max(n_out, 64), 0x5a5a5a5a, dtype=np.uint32)
    keep = [None if a[k] is None else np.ascontiguousarray(a[k]) for k in ("eps2", "epsm2", "w", "s", "rho", "perm", "adj")]
    t0 = time.perf_counter()
    rc = _lib.lib().bluest_mfmc_search(int(a["nb"]), int(a["n_out"]), int(a["flags"]), float(a["budget"]),
                                       *[_lib.ptr(x) for x in keep],
                                       ctypes.byref(mask), _lib.ptr(combo) if outputs_given else None, ctypes.byref(obj),
                                       ctypes.byref(status), None)
    return rc, status.value, mask.value, combo[:n_out].copy(), obj.value, time.perf_counter() - t0


def bits(x):
    return struct.pack("<d", x)


def check(c, repeat=1):
    r = mc.reference(c)
    assert r.rc == c["rc"]
    for _ in range(repeat):
        rc, status, mask, combo, obj, sec = call(c["args"])
        print("%s: rc %d status %d mask %#x obj %r, %.3f s" % (c["name"], rc, status, mask, obj, sec))
        assert rc == r.rc
        if rc: continue
        assert status == r.status
        if status == ref.TOO_BIG: continue                        # nothing else is written
        assert mask == r.best_mask
        assert np.array_equal(combo, r.best_combo)
        assert bits(obj) == bits(r.best_obj), (obj, r.best_obj)


def _ids(group):
    return [c["name"] for c in CASES if c["group"] == group]


def _case(name):
    return next(c for c in CASES if c["name"] == name)


@pytest.fixture(autouse=True, scope="module")
def _library():
    from bluest_amd import build
    build.build()


@pytest.mark.parametrize("name", _ids("base"))
def test_base(name):
    check(_case(name))


@pytest.mark.parametrize("name", _ids("wide"))
def test_wide_sparse_graphs(name):
    """nb >= 21: the scan's grid-stride loop, and winners with a bit at or above 20"""
    check(_case(name))


@pytest.mark.parametrize("name", _ids("window"))
def test_windows(name):
    """more than CAND_CAP candidates: the host loop bisects its windows, `best` tightens them, the winner comes late"""
    check(_case(name))


@pytest.mark.parametrize("name", _ids("round"))
def test_rounding_keeps_the_first_minimum(name):
    """a lane of k_mfmc_round meets two combinations with the same point; best_combo is the lower one"""
    c = _case(name)
    F = mc.reference(c).facts
    assert F["winner_last_minimum_combo"] != F["winner_combo"]      # the table test on the CPU checks this too
    check(c)


@pytest.mark.parametrize("name", _ids("tie"))
def test_ties_go_to_the_earlier_clique(name):
    """two cliques share the best objective bit for bit; five calls give the one answer"""
    check(_case(name), repeat=5)


@pytest.mark.parametrize("name", _ids("small_budget"))
def test_small_budget_pins(name):
    check(_case(name))


@pytest.mark.parametrize("name", _ids("status"))
def test_status(name):
    """NONE, TOO_BIG, and BLUEST_ERR_STATE when more than CAND_CAP cliques share the lower bound zero"""
    c = _case(name)
    check(c)
    if c["rc"]:
        from bluest_amd import _lib
        assert b"counting scans" in _lib.lib().bluest_last_error()      # the scan cap, not the halving limit
        # the bounded window loop: at most MAX_IDLE_SCANS + MAX_HALVINGS scans of 2^18 masks with a host synchronisation
        # each.  profiles/mfmc_search_bench.txt has 5 ms for 2^23 full evaluations, 0.2 ms for 2^18: about 1 s in all; the
        # unbounded loop would take some 5e5 scans, minutes
        assert call(c["args"])[5] < 5.0
        check(mc.valid_small())                                  # a valid call still succeeds afterwards


@pytest.mark.parametrize("name,change", mc.arg_cases(), ids=[n for n, _ in mc.arg_cases()])
def test_argument_checks(name, change):
    """every bad argument is refused before any launch, and a valid call still succeeds afterwards"""
    v = mc.valid_small()
    change = dict(change)
    given = change.pop("outputs_given", True)
    assert call(v["args"], outputs_given=given, **change)[0] == ref.ERR_ARG
    a = dict(v["args"])
    a.update(change)
    assert ref.search(outputs_given=given, **a).rc == ref.ERR_ARG
    check(v)

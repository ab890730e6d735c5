"""
bluest_cov_project bit for bit against a record of the commit before proj()'s eigensolver moved into csrc/jacobi.hpp:
everything a call writes (X, f, gpmax, it, count, info) for the smallest rows that reach each part of the shared routine
(covproj_cases.bits_cases() lists them and says why).  The record, tests/golden/covproj_bits_parent.npz, was written by
tools/gen_golden_covproj_bits.py from that commit on the MI355X; the inputs are seeded, the file holds results only.

np.array_equal throughout (the record is NaN-free): the move changes where the sweeps are written down, never which operations
run in which order.
"""
import os

import numpy as np
import pytest

import covproj_cases as cc
from conftest import golden
from oracle import covproj_ref as ref


@pytest.fixture(scope="module")
def record():
    return golden("covproj_bits_parent.npz")


def test_record_is_complete(record):
    """CPU: every row has its six arrays, within the size a committed fixture may have; no NaN hides a difference"""
    assert sorted(record) == sorted("%s/%s" % (n, k) for n in cc.BITS_NAMES for k in cc.BITS_FIELDS)
    for name in cc.BITS_NAMES:
        M = cc.bits_cases()[cc.BITS_NAMES.index(name)]["C"].shape[0]
        assert record[name + "/X"].shape == (M, M) and record[name + "/X"].dtype == np.float64, name
        for k in cc.BITS_FIELDS:
            a = record["%s/%s" % (name, k)]
            assert a.size > 0 and not np.isnan(a.astype(np.float64)).any(), (name, k)
        spg = name.startswith("spg")
        assert int(record[name + "/info"]) == (ref.MAXIT if spg else ref.OK), name
        assert int(record[name + "/it"]) == (3 if spg else 0), name
    assert os.path.getsize(os.path.join(os.path.dirname(__file__), "golden", "covproj_bits_parent.npz")) < 400 * 1024


def test_rows_reach_their_parts():
    """CPU: the sizes the rows are there for"""
    sizes = [r["C"].shape[0] for r in cc.bits_cases()]
    assert {2, 3, 4, 31, 32, 64} <= set(sizes) and any(r["group"] == "spg" and r["params"]["maxit"] == 3 for r in cc.bits_cases())
    h = 64 // 2
    assert h * (h + 1) // 2 == 528 > 256
    ov = cc.overflow_case()["C"]
    with np.errstate(over="ignore"):
        assert np.isinf((ov ** 2).sum()) and np.isfinite(ov).all()


@pytest.mark.gpu
@pytest.mark.parametrize("name", cc.BITS_NAMES)
def test_covproj_bits(record, name):
    import torch
    import test_gpu_covproj_abi as abi
    assert torch.cuda.is_available(), "these tests need the MI355X"
    got = cc.bits_record(abi.solo, cc.bits_cases()[cc.BITS_NAMES.index(name)])
    for key, a in got.items():
        want = record[key]
        assert a.dtype == want.dtype and a.shape == want.shape, key
        print("%-36s %6d entries, %d differ" % (key, a.size, int((a != want).sum())))
        assert np.array_equal(a, want), key

"""
The sampling and pilot mix-ins against the bit record tests/golden/sampling_mixins.npz (tools/gen_golden_sampling_mixins.py, which
also says what is in it): the toy problems of the host tests are built again, with the numpy restatements standing in for the GPU
wrappers, and every returned array, every report and every list of sampler calls must be what the record holds, bit for bit.
The other host tests compare twins with each other and hold several of these results to a tolerance only; this one pins them.
"""
import importlib.util
import os

import numpy as np

from conftest import GOLDEN, ROOT
from gsums_ref import same_bits


def _generator():
    spec = importlib.util.spec_from_file_location("gen_golden_sampling_mixins", os.path.join(ROOT, "tools", "gen_golden_sampling_mixins.py"))
    module = importlib.util.module_from_spec(spec)
    spec.loader.exec_module(module)
    return module


def test_every_recorded_bit_and_call_is_reproduced():
    want = dict(np.load(os.path.join(GOLDEN, "sampling_mixins.npz")))
    got = _generator().record()
    assert sorted(got) == sorted(want) and len(want) > 300
    for key in sorted(want):
        if want[key].dtype.kind in "iu":                                # sampler calls, group lists, printed text
            assert got[key].dtype == want[key].dtype and np.array_equal(got[key], want[key]), key
        else:
            assert same_bits(got[key], want[key]), key
    # the record covers what it is meant to cover: both flush sizes, every variant of the field problem, both pilots growing
    for flush in ("default", "each"):
        for problem in ("scalar_batched", "field_plain", "field_stream0", "field_stream13440", "field_cov"):
            assert "%s/%s/vt" % (problem, flush) in want and "%s/%s/sampled" % (problem, flush) in want
    assert same_bits(want["field_stream0/each/mus1"], want["field_plain/each/mus1"])
    for name in ("pilot_tol", "field_pilot_tol"):
        assert want[name + "/report"][1] >= 2 and want[name + "/report"][3] == 1       # rounds, converged
    assert want["pilot_capped/report"][3] == 0 and want["pilot_capped/printed"].size > 0
    assert want["field_pilot_capped_bytes/report"][4] == 2 and want["field_pilot_capped_samples/report"][4] == 1

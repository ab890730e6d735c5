"""
The cross-lane reductions without the LDS crossbar (csrc/common.hpp: wave_sum_dpp, wave_max_dpp, wave_sum_ll_dpp, the fold's
quad_x1 / quad_x2) seen lane by lane through bluest_wave_reduce_probe: one wavefront per row of 64 doubles, every lane's result
written out.

Reference: the xor butterfly they replace, restated in numpy float64 -- y = y + y[:, lane ^ off] for off = 32, 16, 8, 4, 2, 1.  Every
step is one IEEE addition (or maximum) per lane, so the comparison is exact: no tolerance.  What is asserted per row: all 64
lanes hold the same bits, and those bits are the reference's.  The maximum's reference orders zeros as v_max_f64 does (+0 above
-0).  (A NaN of the sum is compared as "NaN in both": payload and sign of a NaN are the adder's choice, not the tree's, and differ
between the host's and the GPU's adders; the lanes of a row still have to agree bit for bit.)

Before the GPU is touched the data are shown to tell pairing trees apart: the ascending level order, levels 4 and 2 swapped, and
half-mirror pairing at level 4 each differ from the right tree in at least a quarter of the random rows.
"""
import ctypes

import numpy as np
import pytest

LANES = np.arange(64)
OFFS = (32, 16, 8, 4, 2, 1)
N_RANDOM = 4096


def tree(x, op, partners):
    y = x.copy()
    with np.errstate(invalid="ignore", over="ignore"):
        for p in partners:
            y = op(y, y[:, p])
    return y


def xor_partners(offs=OFFS):
    return [LANES ^ off for off in offs]


def half_mirror_at_4():
    """level 4 pairs lane i of an 8-lane half row with lane 7 - i (row_half_mirror) instead of i ^ 4"""
    p = xor_partners()
    p[3] = (LANES & ~7) | (7 - (LANES & 7))
    return p


def data():
    rng = np.random.RandomState(20240611)
    rnd = rng.randn(N_RANDOM, 64) * 2.0 ** rng.randint(-30, 31, size=(N_RANDOM, 64))
    sp = []
    sp.append(np.zeros(64))                                             # +0 everywhere
    sp.append(-np.zeros(64))                                            # -0 everywhere: the sum is -0
    z = np.zeros(64); z[::2] = -0.0; sp.append(z)                       # mixed zeros: +0
    z = -np.zeros(64); z[37] = 0.0; sp.append(z)                        # one +0 among -0
    r = rng.randn(64); r[5] = np.inf; sp.append(r)                      # +inf in one lane
    r = rng.randn(64); r[40] = -np.inf; sp.append(r)                    # -inf in one lane
    r = rng.randn(64); r[3] = np.inf; r[60] = -np.inf; sp.append(r)     # inf - inf: NaN made by the tree
    r = rng.randn(64); r[17] = np.nan; sp.append(r)                     # NaN in one lane
    sp.append(rng.randn(64) * 5e-324 * 2.0 ** rng.randint(0, 40, 64))   # denormals
    sp.append(np.full(64, 5e-324))                                      # 64 x the smallest denormal
    r = rng.randn(64); r[32:] = -r[:32]; sp.append(r)                   # exact cancellation at the first level
    r = rng.randn(64); r[1::2] = -r[0::2]; sp.append(r)                 # ... only at the last level
    r = np.full(64, 1.0); r[0] = 2.0 ** 60; r[33] = -2.0 ** 60; sp.append(r)      # large terms that cancel late
    r = -np.abs(rng.randn(64)) - 1.0; sp.append(r)                      # maximum of negative numbers
    return rnd, np.array(sp)


def fmax_hw(a, b):
    """fmax as v_max_f64 orders zeros: max(+0, -0) = +0 whichever operand comes first (numpy leaves that sign to the platform);
    a NaN operand is ignored, as in fmax"""
    r = np.fmax(a, b)
    both_zero = (a == 0.0) & (b == 0.0)
    return np.where(both_zero, np.where(np.signbit(a) & np.signbit(b), -0.0, 0.0), r)


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64)


def same(a, b):
    """equal bits, a NaN matching any NaN"""
    return (bits(a) == bits(b)) | (np.isnan(a) & np.isnan(b))


def test_data_tell_trees_apart():
    """CPU: the random rows distinguish the right tree from its plausible mistakes in at least a quarter of the rows each"""
    rnd, _ = data()
    right = tree(rnd, np.add, xor_partners())
    wrong = {"ascending": xor_partners(OFFS[::-1]), "levels 4 and 2 swapped": xor_partners((32, 16, 8, 2, 4, 1)),
             "half mirror at level 4": half_mirror_at_4()}
    for name, partners in wrong.items():
        other = tree(rnd, np.add, partners)
        frac = float((bits(other[:, 0]) != bits(right[:, 0])).mean())
        print("%-24s differs in %.0f %% of the rows" % (name, 100 * frac))
        assert frac >= 0.25, (name, frac)
    # every lane of the reference itself holds the same bits (commutative additions on one tree)
    assert (bits(right) == bits(right[:, :1])).all()


@pytest.mark.gpu
def test_every_lane_against_the_butterfly():
    import torch
    from bluest_amd import _lib
    assert torch.cuda.is_available(), "this test needs the MI355X"
    rnd, sp = data()
    x = np.concatenate([rnd, sp])
    n = len(x)
    dev = torch.device("cuda", torch.cuda.current_device())
    xd = torch.from_numpy(x).to(dev)
    out = [torch.empty((n, 64), dtype=torch.float64, device=dev) for _ in range(3)]
    iout = torch.empty((n, 64), dtype=torch.int64, device=dev)
    _lib.check(_lib.lib().bluest_wave_reduce_probe(xd.data_ptr(), n, out[0].data_ptr(), out[1].data_ptr(), out[2].data_ptr(),
                                                  iout.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    s, mx, q = (t.cpu().numpy() for t in out)
    isum = iout.cpu().numpy()
    ref_s = tree(x, np.add, xor_partners())
    ref_q = tree(x, np.add, xor_partners((1, 2)))
    ref_m = tree(x, fmax_hw, xor_partners())
    ref_i = tree(x.view(np.int64) >> 8, np.add, xor_partners())
    for name, got, ref in (("sum", s, ref_s), ("quad", q, ref_q)):
        bad = ~same(got, ref)
        print("%-5s rows with a wrong lane: %d of %d (random %d, special %s)" % (name, bad.any(axis=1).sum(), n, bad[:N_RANDOM].any(axis=1).sum(),
                                                                                  np.flatnonzero(bad[N_RANDOM:].any(axis=1)).tolist()))
    # all lanes of a row agree bit for bit (sum, max, integer sum over the wave; the quad sum over each quad)
    assert (bits(s) == bits(s[:, :1])).all()
    assert (bits(mx) == bits(mx[:, :1])).all()
    assert (isum == isum[:, :1]).all()
    q4 = bits(q).reshape(n, 16, 4)
    assert (q4 == q4[:, :, :1]).all()
    # ... and they are the butterfly's bits
    assert same(s, ref_s).all()
    assert same(q, ref_q).all()
    assert np.array_equal(isum, ref_i)
    # maximum: bits again, with the rule of v_max_f64 for zeros (+0 above -0) in the reference
    assert same(mx, ref_m).all()

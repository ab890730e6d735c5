"""
wave_sum_multi (csrc/common.hpp), the reduction of OB = 2, 4 or 8 wave sums at once in the tail of k_phi_chunks_shared, seen through
bluest_wave_reduce_multi_probe: one wavefront per group of OB rows of 64 doubles, every total written by the lane that stores it in
the kernel.  Its first two levels exchange halves and rows of DIFFERENT registers, so what can go wrong that a single sum cannot:
a total ends in another output's place, or the levels 32 and 16 change places.

Data: the 4 096 random rows and the 14 special rows of tests/test_gpu_wave_reduce.py (zeros of both signs, infinities, inf - inf,
NaN, denormals, early and late cancellation), taken OB at a time; every special row has one turn in every output position, among
random neighbours.  Reference: the xor butterfly of that file in numpy float64, lane 0 of it.  Equal bits, a NaN matching a NaN
(payload and sign of a NaN are the adder's choice, not the tree's).

Before the GPU is touched the data are shown to tell the two mistakes apart from the right result in at least a quarter of the
random rows each.
"""
import ctypes

import numpy as np
import pytest

import test_gpu_wave_reduce as wr

OBS = (2, 4, 8)


def groups(ob):
    """(n_groups, ob, 64): the random rows ob at a time, then each special row at each of the ob positions"""
    rnd, sp = wr.data()
    g = [rnd.reshape(-1, ob, 64)]
    fill = 0
    for row in sp:
        for pos in range(ob):
            grp = np.empty((ob, 64))
            for oo in range(ob):
                if oo == pos:
                    grp[oo] = row
                else:
                    grp[oo] = rnd[fill % len(rnd)]
                    fill += 1
            g.append(grp[None])
    return np.concatenate(g), len(rnd) // ob


def reference(x):
    """(n_groups, ob) butterfly totals"""
    n, ob, _ = x.shape
    return wr.tree(x.reshape(n * ob, 64), np.add, wr.xor_partners())[:, 0].reshape(n, ob)


def test_data_tell_mistakes_apart():
    """CPU: two outputs' results exchanged, or level 16 paired before level 32, differ from the right totals in at least a
    quarter of the random rows"""
    rnd, _ = wr.data()
    right = wr.tree(rnd, np.add, wr.xor_partners())[:, 0]
    early16 = wr.tree(rnd, np.add, wr.xor_partners((16, 32, 8, 4, 2, 1)))[:, 0]
    frac = float((wr.bits(early16) != wr.bits(right)).mean())
    print("level 16 before level 32 differs in %.0f %% of the rows" % (100 * frac))
    assert frac >= 0.25, frac
    for ob in OBS:
        x, n_rnd = groups(ob)
        ref = reference(x)[:n_rnd]
        for d in (1, ob // 2):                       # neighbours, and the two halves of the block
            swapped = ref[:, np.arange(ob) ^ d]
            frac = float((wr.bits(swapped) != wr.bits(ref)).mean())
            print("OB = %d: outputs oo and oo ^ %d exchanged differ in %.0f %% of the rows" % (ob, d, 100 * frac))
            assert frac >= 0.25, (ob, d, frac)
    # every special row sits once at every position
    _, sp = wr.data()
    for ob in OBS:
        x, n_rnd = groups(ob)
        tail = x[n_rnd:].reshape(len(sp), ob, ob, 64)
        for i, row in enumerate(sp):
            for pos in range(ob):
                assert wr.bits(tail[i, pos, pos]).tolist() == wr.bits(row).tolist()


@pytest.mark.gpu
@pytest.mark.parametrize("ob", OBS)
def test_totals_against_the_butterfly(ob):
    import torch
    from bluest_amd import _lib
    assert torch.cuda.is_available(), "this test needs the MI355X"
    x, n_rnd = groups(ob)
    n = len(x)
    ref = reference(x)
    dev = torch.device("cuda", torch.cuda.current_device())
    xd = torch.from_numpy(np.ascontiguousarray(x)).to(dev)
    out = torch.full((n, ob), 1.2345e300, dtype=torch.float64, device=dev)      # (no total of these data)
    _lib.check(_lib.lib().bluest_wave_reduce_multi_probe(xd.data_ptr(), n, ob, out.data_ptr(),
                                                        ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    got = out.cpu().numpy()
    bad = ~wr.same(got, ref)
    print("OB = %d: %d groups, wrong totals: %d (random groups %d, special groups %s)" %
          (ob, n, bad.sum(), bad[:n_rnd].sum(), np.flatnonzero(bad[n_rnd:].any(axis=1)).tolist()))
    assert not (got == 1.2345e300).any()
    assert wr.same(got, ref).all()

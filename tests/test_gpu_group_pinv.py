"""
GPU tests (-m gpu) of the per-group pseudo-inverse kernels, k_group_pinv<K, G> (K = 1..16, one thread per group) and
k_group_pinv_wide<G> (K = 17..32, one wavefront per group), in both instantiations of the group list: int64 through
bluest_group_pinv and uint8 through the set-up of a Plan built from a covariance, read back through plan.invcovs.  The reference is
the 80-bit Jacobi pseudo-inverse of pinv_ref.py on the case table of pinv_cases.py, which test_pinv_ref.py admits on the CPU.

Errors are norm(got - want) / norm(want) (Frobenius).  Wishart blocks: 1e-12, the tolerance of the tests before these.  Every other
kind: 100 cond_kept eps, cond_kept from the 80-bit eigenvalues and 100 from test_group_pinv_wide_vs_numpy.  Diagonal blocks and the
power-of-two scale: bit equality.  Every test prints its largest error / bound (profiles/pinv_tests_gpu.txt keeps them).
"""
import numpy as np
import pytest

import pinv_cases as pc
import pinv_ref as ref

pytestmark = pytest.mark.gpu


@pytest.fixture(scope="module")
def gpu():
    import torch
    from bluest_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert _lib.device_count() >= 1
    return torch


def _run(index, C, K, groups):
    """(Lk, K, K) pseudo-inverses of C[g, g] through the int64 or the uint8 instantiation"""
    from bluest_amd import misc
    from bluest_amd.plan import Plan
    groups = np.ascontiguousarray(groups, dtype=np.int64).reshape(-1, K)
    Lk, N = len(groups), C.shape[0]
    if index == "int64":
        return misc.group_pinv(C, K, groups).reshape(Lk, K, K)
    assert N <= 64
    plan = Plan(N, Lk, [{"K": K, "sizes": [0] * (K - 1) + [Lk], "groups": [np.zeros((0, j), dtype=np.int64) for j in range(1, K)] + [groups],
                         "C": C, "mapping": None}])
    return np.asarray(plan.invcovs[0]).reshape(Lk, K, K).copy()


def _check_call(call, got, K, index, ratios):
    for i, row in enumerate(call.rows):
        r = pc.row_reference(row)
        assert np.isfinite(got[i]).all(), row.name
        if r["exact"] is not None:                       # a diagonal block: no rotation happens, 1 / d_i and exact zeros
            assert np.array_equal(got[i], r["exact"]), (row.name, np.abs(got[i] - r["exact"]).max())
            continue
        err = ref.fro_err(got[i], r["pinv"])
        ratios[row.kind] = max(ratios.get(row.kind, 0.0), err / r["tol"])
        print("  %-28s cond %.1e  err %.2e  bound %.2e" % (row.name, r["cond"], err, r["tol"]))
        assert err <= r["tol"], (row.name, err, r["tol"], r["cond"])


def _report(what, K, index, ratios):
    for kind, x in sorted(ratios.items()):
        print("PINV_RATIO %s K=%d %s %s %.3e" % (what, K, index, kind, x))


@pytest.mark.parametrize("index", pc.INDEX_TYPES)
@pytest.mark.parametrize("K", pc.KS)
def test_blocks_vs_reference(gpu, K, index):
    """every kind of block that K admits, two of each, against the 80-bit reference; the first call is made twice and gives the
    same bits"""
    ratios = {}
    for n, call in enumerate(pc.calls_of(K, index)):
        got = _run(index, call.C, K, call.groups)
        if n == 0:
            assert np.array_equal(got, _run(index, call.C, K, call.groups)), "two calls on the same input differ"
        _check_call(call, got, K, index, ratios)
        # an unsorted group against the same models sorted, in the same covariance: the permuted answer.  Each side lies within
        # the bound of the exact answer, so the two lie within twice the bound of each other
        uns = [i for i, row in enumerate(call.rows) if row.kind == "unsorted"]
        if uns:
            gs = np.sort(call.groups[uns], axis=1)
            srt = _run(index, call.C, K, gs)
            for j, i in enumerate(uns):
                perm = np.searchsorted(gs[j], call.groups[i])
                assert not np.array_equal(perm, np.arange(K)), call.rows[i].name
                err = ref.fro_err(got[i], srt[j][np.ix_(perm, perm)])
                ratios["unsorted_vs_sorted"] = max(ratios.get("unsorted_vs_sorted", 0.0), err / (2 * pc.WISHART_TOL))
                assert err <= 2 * pc.WISHART_TOL, (call.rows[i].name, err)
    _report("blocks", K, index, ratios)


@pytest.mark.parametrize("index", pc.INDEX_TYPES)
@pytest.mark.parametrize("K", sorted(pc.NARROW_EDGES) + sorted(pc.WIDE_EDGES))
def test_launch_edges(gpu, K, index):
    """Lk around the block size of k_group_pinv (64 threads, one group each) and more than one workgroup of the wide kernel: a
    call of Lk groups drawn cyclically from a small pool, with the pool's first group also put in the middle and at the end,
    gives for every group the bits that the pool alone gives, and those are pseudo-inverses"""
    C, pool = pc.edge_pool(K)
    base = _run(index, C, K, pool)
    worst = 0.0
    for i, g in enumerate(pool):
        err = ref.fro_err(base[i], ref.pinv_ld(C[np.ix_(g, g)])[0])
        worst = max(worst, err / pc.WISHART_TOL)
        assert err <= pc.WISHART_TOL, (K, index, i, err)
    print("PINV_RATIO edges K=%d %s wishart %.3e" % (K, index, worst))
    for Lk in (pc.NARROW_EDGES.get(K) or pc.WIDE_EDGES[K]):
        idx = np.arange(Lk) % len(pool)
        idx[Lk // 2] = 0
        idx[-1] = 0
        got = _run(index, C, K, pool[idx])
        assert got.shape == (Lk, K, K)
        bad = [i for i in range(Lk) if not np.array_equal(got[i], base[idx[i]])]
        assert not bad, (K, index, Lk, bad[:10])


@pytest.mark.parametrize("K", pc.BIG_KS)
def test_int64_indices_beyond_a_byte(gpu, K):
    """N = 300 and model indices up to 299 on the int64 path: against the reference, and the same bits as the same block in a
    covariance of K models"""
    C, groups = pc.big_index_case(K)
    got = _run("int64", C, K, groups)
    worst = 0.0
    for i, g in enumerate(groups):
        sub = np.ascontiguousarray(C[np.ix_(g, g)])
        err = ref.fro_err(got[i], ref.pinv_ld(sub)[0])
        worst = max(worst, err / pc.WISHART_TOL)
        assert err <= pc.WISHART_TOL, (K, i, err)
        assert np.array_equal(got[i], _run("int64", sub, K, np.arange(K))[0]), (K, i)
    print("PINV_RATIO big_index K=%d int64 wishart %.3e" % (K, worst))


@pytest.mark.parametrize("index", pc.INDEX_TYPES)
@pytest.mark.parametrize("K", pc.SCALE_KS)
def test_power_of_two_scale(gpu, K, index):
    """pinv(2^515 C) == 2^-515 pinv(C) and pinv(2^-540 C) == 2^540 pinv(C), bit for bit, on every kind of block: every operation
    commutes with a power-of-two scale as long as nothing over- or underflows, and at these magnitudes the square of an entry
    does (inf, or 0).  The unscaled side is checked against the reference."""
    ratios, diff = {}, {}
    for call in pc.calls_of(K, index):
        base = _run(index, call.C, K, call.groups)
        _check_call(call, base, K, index, ratios)
        for e in pc.SCALES:
            Cs = np.ldexp(call.C, e)
            assert np.isfinite(Cs).all() and np.array_equal(np.ldexp(Cs, -e), call.C)
            got = _run(index, Cs, K, call.groups)
            want = np.ldexp(base, -e)                    # exact: far from the subnormals and from overflow
            assert np.isfinite(want).all() and np.array_equal(np.ldexp(want, e), base)
            for i, row in enumerate(call.rows):
                diff[(e, row.kind)] = diff.get((e, row.kind), 0) + int((got[i] != want[i]).sum())
    for (e, kind), n in sorted(diff.items()):
        print("PINV_SCALE K=%d %s 2^%d %s: %d entries differ" % (K, index, e, kind, n))
    _report("scale_base", K, index, ratios)
    assert not any(diff.values()), {k: v for k, v in diff.items() if v}

"""
GPU tests (-m gpu) of k_pinv_from_record through bluest_plan_solve_pinv, fed directly: a minimal plan (singletons only, 3 outputs,
2 candidates) for N in {1, 2, 5, 33, 54, 55, 64} (the dynamic LDS crosses 48 KiB between 54 and 55), records [2][3][N*N + 2N + 1]
filled by hand from the record rows of pinv_cases.py, and V, v and the status compared with pinv_ref.record_pinv, the 80-bit
restatement of what the kernel documents.  The six (candidate, output) slots of a launch hold different matrices, so an indexing
slip shows; the buffers are longer than the kernel may write and the tails are poisoned.

V is measured relative to |V| and v relative to its largest entry; both bounds are 100 cond_kept eps, cond_kept from the 80-bit
eigenvalues of the pass that gives the value.  Entries of v outside mask2 are exactly zero.  The power-of-two scale: bit equality.
"""
import numpy as np
import pytest

import pinv_cases as pc
import pinv_ref as ref

pytestmark = pytest.mark.gpu

PAD, POISON, POISON_I = 37, -1.2345e300, -77
_PLANS = {}


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _plan(N):
    from bluest_amd.plan import Plan
    if N not in _PLANS:
        out = {"K": 1, "sizes": [N], "groups": [np.arange(N, dtype=np.int64).reshape(N, 1)], "invcovs": [np.ones(N)], "mapping": None}
        _PLANS[N] = Plan(N, N, [dict(out) for _ in range(pc.N_OUT)], max_candidates=pc.N_CAND)
    return _PLANS[N]


def _solve_pinv(torch, N, recs, delta):
    """V (6,), v (6, N), status (6,) of the records (6, reclen), slot = candidate * 3 + output; checks the poisoned tails"""
    from bluest_amd._lib import check
    from bluest_amd.plan import _stream
    plan = _plan(N)
    n = pc.N_OUT * pc.N_CAND
    recs = np.ascontiguousarray(recs, dtype=np.float64)
    assert recs.shape == (n, ref.record_len(N)) and plan.reclen == ref.record_len(N)
    rec = torch.from_numpy(recs).to(plan.device)
    var = torch.from_numpy(np.full(n + PAD, POISON)).to(plan.device)
    v = torch.from_numpy(np.full(n * N + PAD, POISON)).to(plan.device)
    status = torch.from_numpy(np.full(n + PAD, POISON_I, dtype=np.int32)).to(plan.device)
    with torch.cuda.device(plan.device):
        check(plan.lib.bluest_plan_solve_pinv(plan._h, rec.data_ptr(), pc.N_CAND, float(delta), var.data_ptr(), v.data_ptr(),
                                              status.data_ptr(), _stream()))
        torch.cuda.synchronize()
    var, v, status = var.cpu().numpy(), v.cpu().numpy(), status.cpu().numpy()
    assert np.array_equal(var[n:], np.full(PAD, POISON)) and np.array_equal(v[n * N:], np.full(PAD, POISON))
    assert np.array_equal(status[n:], np.full(PAD, POISON_I, dtype=np.int32))
    assert np.array_equal(rec.cpu().numpy(), recs), "the records were written to"
    return var[:n].copy(), v[:n * N].reshape(n, N).copy(), status[:n].copy()


def _launch(N, launch):
    rows = pc.launch_rows(N, launch)
    refs = [pc.record_reference(r.name) for r in rows]
    return rows, refs, np.stack([r["rec"] for r in refs]), pc.LAUNCHES[launch][0]


@pytest.mark.parametrize("launch", list(pc.LAUNCHES))
@pytest.mark.parametrize("N", pc.RECORD_NS)
def test_records_vs_reference(gpu, N, launch):
    """six different records per launch: regular, rank-deficient by 1, 2 and N/2, null directions with unsampled models (whose
    rows hold noise), model 0 unsampled with and without a singular Phi, two passes on a singular Phi with delta = 1e-3, an
    asymmetric record, big = 0 and all flags zero; two launches give the same bits"""
    rows, refs, recs, delta = _launch(N, launch)
    V, v, st = _solve_pinv(gpu, N, recs, delta)
    V2, v2, st2 = _solve_pinv(gpu, N, recs, delta)
    assert np.array_equal(V, V2, equal_nan=True) and np.array_equal(v, v2) and np.array_equal(st, st2)
    ratios = {}
    for s, (row, r) in enumerate(zip(rows, refs)):
        assert st[s] == r["status"], (row.name, s, st[s], r["status"])
        if not r["w"]:
            assert (np.isposinf(V[s]) if r["status"] == ref.EVAL_INF else np.isnan(V[s])) and not np.any(v[s]), (row.name, V[s])
            continue
        eV, ev = ref.max_err(V[s], r["V"]), ref.max_err(v[s], r["v"])
        print("  %-30s slot %d  V err %.2e bound %.2e   v err %.2e bound %.2e" % (row.name, s, eV, r["tolV"], ev, r["tolv"]))
        ratios[row.kind] = max(ratios.get(row.kind, 0.0), eV / r["tolV"], ev / r["tolv"])
        assert np.isfinite(V[s]) and np.isfinite(v[s]).all(), row.name
        assert eV <= r["tolV"], (row.name, s, eV, r["tolV"])
        assert ev <= r["tolv"], (row.name, s, ev, r["tolv"])
        assert not np.any(v[s][np.asarray(r["v"]) == 0]), (row.name, "v is not zero outside mask2")
    for kind, x in sorted(ratios.items()):
        print("PINV_RATIO record N=%d %s %s %.3e" % (N, launch, kind, x))


@pytest.mark.parametrize("launch", [k for k, (d, _) in pc.LAUNCHES.items() if d == 0.0])
@pytest.mark.parametrize("N", pc.RECORD_NS)
def test_record_power_of_two_scale(gpu, N, launch):
    """delta = 0: the record of 2^e Phi gives 2^-e V and 2^-e v, bit for bit, at e = 515 and e = -540, and the same status"""
    rows, refs, recs, delta = _launch(N, launch)
    V, v, st = _solve_pinv(gpu, N, recs, delta)
    bad = []
    for e in pc.SCALES:
        scaled = recs.copy()
        scaled[:, :N * N] = np.ldexp(recs[:, :N * N], e)
        assert np.isfinite(scaled).all() and np.array_equal(np.ldexp(scaled[:, :N * N], -e), recs[:, :N * N])
        Vs, vs, sts = _solve_pinv(gpu, N, scaled, delta)
        assert np.array_equal(sts, st), (N, launch, e)
        for s, row in enumerate(rows):
            nV = int(not np.array_equal(Vs[s], np.ldexp(V[s], -e), equal_nan=True))
            nv = int((vs[s] != np.ldexp(v[s], -e)).sum())
            print("PINV_SCALE record N=%d %s 2^%d %-26s V differs: %d, v entries differing: %d of %d" % (N, launch, e, row.name, nV, nv, N))
            if nV or nv:
                bad.append((e, row.name, nV, nv))
    assert not bad, bad

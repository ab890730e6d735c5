"""
The two evaluation paths that run with more dynamic LDS than a default launch grants (48 KiB): the pseudo-inverse fall-back of a
rank-deficient Phi (k_pinv_from_record, 2 N (N+1) doubles: 66 560 B at N = 64) and the _cmisc_bluest mirrors at wide groups
(k_objectiveK, N^2 doubles: 128 KiB at N = 128), each against a plain restatement: the 80-bit reference (oracle/ld_eval.py) and
numpy's pinv, or the oracle's C restatement of cmisc.cpp (oracle/bluest_oracle.c).
"""
import numpy as np
import pytest

from bluest_amd import synth
from conftest import rel_err
from oracle import ld_eval

pytestmark = pytest.mark.gpu
EPS = ld_eval.EPS


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def _rank_deficient_plan(n, n_out, rng):
    """a plan whose Phi is exactly rank-deficient: models a = n-2 and b = n-1 are one model twice -- they only ever appear
    together, in the one group {a, b} whose inverse is the rank-one pseudo-inverse 0.5 [[1, 1], [1, 1]] -- so e_a - e_b spans the
    null space of every term.  Every other block is the float64 inverse of a Wishart block."""
    a, b = n - 2, n - 1
    singles = np.arange(n - 2).reshape(-1, 1)
    allp = synth.all_groups(n - 2, 2)[1]
    pairs = allp[np.sort(rng.choice(len(allp), min(len(allp), 300), replace=False))]
    pairs = np.concatenate([pairs, [[a, b]]]).astype(np.int64)
    triples = np.array(sorted({tuple(sorted(rng.choice(n - 2, 3, replace=False).tolist())) for _ in range(150)}), dtype=np.int64)
    G = [singles, pairs, triples]
    outs, blocks = [], []
    for o in range(n_out):
        C = synth.wishart_covariance(n, o)[0]
        ic = []
        for k, g in enumerate(G, start=1):
            B = np.linalg.inv(C[g[:, :, None], g[:, None, :]])
            if k == 2:
                B[-1] = 0.5                                           # the {a, b} group
            ic.append(B.reshape(-1))
        outs.append({"K": 3, "sizes": [len(g) for g in G], "groups": G, "invcovs": ic, "mapping": None})
        blocks.append(ld_eval.blocks_from_flat([len(g) for g in G], np.concatenate(ic)))
    return G, outs, blocks


@pytest.mark.parametrize("n", [40, 55, 64])
def test_pinv_fallback_at_full_width(gpu, n):
    """eval_pinv on an exactly rank-deficient Phi, 3 outputs, 2 candidates, delta = 0 and delta != 0, against the 80-bit
    reference (pinv of a block-diagonal matrix = the inverse of its regular block, zero on the null block: models a, b leave V's
    system and y) and numpy's pinv of the float64 matrix."""
    torch = gpu
    from bluest_amd.plan import Plan
    rng = np.random.RandomState(n)
    G, outs, blocks = _rank_deficient_plan(n, 3, rng)
    L = sum(len(g) for g in G)
    plan = Plan(n, L, outs, max_candidates=2)
    M = np.stack([0.5 + rng.rand(L), 0.5 + 2 * rng.rand(L)])
    Md = torch.from_numpy(M).to(plan.device)
    _, _, st = plan.eval(Md)
    assert (st.cpu().numpy() == 3).all()                             # the elimination refuses it: this is the fall-back's case
    keep = [np.ones(len(g), bool) for g in G]
    keep[1][-1] = False                                              # the regular block: every group but {a, b}
    Greg = [g[kk] for g, kk in zip(G, keep)]
    sel = np.concatenate(keep)
    for delta in (0.0, 1e-3):
        var, grad, st = plan.eval_pinv(Md, delta=delta)
        var, grad, st = var.cpu().numpy(), grad.cpu().numpy(), st.cpu().numpy()
        assert (st == 0).all()
        for c in range(2):
            for o in range(3):
                if delta == 0.0:
                    Bo = [B[kk] for B, kk in zip(blocks[o], keep)]
                    r = ld_eval.evaluate(n, Greg, Bo, M[c][sel])
                    want_g = np.zeros(L)
                    want_g[sel] = r["grad"]                          # y vanishes on a and b: the {a, b} entry is -0
                else:
                    r = ld_eval.evaluate(n, G, blocks[o], M[c], delta=delta)
                    want_g = r["grad"]
                # Jacobi eigen-decomposition: residual ~ N eps |Phi|, so V and y move by cond(non-zero part) N eps; the
                # eigenvalue cut 1e-15 max|lambda| lies far below the smallest kept one (cond ~ 1e5 << 1e15).  Tighter than the
                # 1e-9 of test_pinv_path_equals_the_elimination wherever cond < 1e5
                tol = 4 * n * r["cond"] * EPS
                assert abs(var[c, o] / r["V"] - 1) <= tol, (n, delta, c, o, var[c, o], r["V"], tol)
                assert rel_err(grad[c, plan.grad_off[o]:plan.grad_off[o] + L], want_g) <= 2 * tol, (n, delta, c, o)
                if delta == 0.0:
                    P = ld_eval.phi_ld(n, G, blocks[o], M[c]).astype(np.float64)
                    assert abs(var[c, o] / np.linalg.pinv(P)[0, 0] - 1) <= 2 * tol


def _rand_groups(N, k, Lk, rng):
    return np.array([np.sort(rng.choice(N, k, replace=False)) for _ in range(Lk)], dtype=np.int64).reshape(Lk, k)


def _rand_inv(k, Lk, rng):
    A = rng.randn(Lk, k, k + 2)
    return np.ascontiguousarray(np.linalg.inv(A @ A.transpose(0, 2, 1) / (k + 2)).reshape(-1))


@pytest.mark.parametrize("N", [20, 64, 128])
def test_cmisc_mirrors_wide_groups(gpu, oracle, N):
    """assemble_psi, objectiveK (float64 and int64 m), gradK, cleanupK, hessKQ for k, q in {1, 5, 12, 17, 32} (k, q <= N) against
    the oracle's C restatement of cmisc.cpp, through host pointers, device pointers and the += contract of the native module.
    Bounds, relative to the largest entry: objectiveK adds Lk k^2 products into N^2 entries with LDS atomics (any order):
    Lk k^2 eps; gradK / hessKQ sum k^2 / k q products per entry in another order than the C loop: k^2 (k q) eps times the
    spread sum|t| / |sum t| (<= 10 for these positive definite blocks)."""
    torch = gpu
    from bluest_amd import _lib, misc
    rng = np.random.RandomState(N)
    P = rng.randn(N, N)
    P = P @ P.T / N
    Lk = 40
    ks = [k for k in (1, 5, 12, 17, 32) if k <= N]
    data = {k: (_rand_groups(N, k, Lk, rng), _rand_inv(k, Lk, rng), 0.5 + rng.rand(Lk), rng.randint(1, 50, Lk).astype(np.int64)) for k in ks}
    for k in ks:
        g, ic, mk, mi = data[k]
        bound = k * k * EPS * Lk
        if N <= 64:                                                  # psi is N^2 x Lk: 5 MB at N = 128, left out
            assert rel_err(misc.assemble_psi(N, k, Lk, g, ic), oracle.assemble_psi(N, k, Lk, g, ic)) == 0.0
        assert rel_err(misc.objectiveK(N, k, Lk, mk, g, ic), oracle.objectiveK(N, k, Lk, mk, g, ic)) <= bound, k
        assert rel_err(misc.objectiveK(N, k, Lk, mi, g, ic), oracle.objectiveK(N, k, Lk, mi, g, ic)) <= bound, k
        assert rel_err(misc.gradK(k, Lk, g, ic, P), oracle.gradK(k, Lk, g, ic, P)) <= 10 * k * k * EPS, k
        assert rel_err(misc.cleanupK(k, Lk, g, ic, P), oracle.cleanupK(k, Lk, g, ic, P)) == 0.0, k
        for q in ks:
            gq, icq, _, _ = data[q]
            assert rel_err(misc.hessKQ(k, q, Lk, Lk, g, gq, ic, icq, P),
                           oracle.hessKQ(k, q, Lk, Lk, g, gq, ic, icq, P)) <= 10 * 2 * k * q * EPS * max(k, q), (k, q)
    # += contract and device pointers at the widest group
    k = ks[-1]
    g, ic, mk, _ = data[k]
    want = oracle.objectiveK(N, k, Lk, mk, g, ic)
    PHI = np.ones(N * N)
    misc.objectiveK_c(PHI, N, k, Lk, mk, g.ravel(), ic)
    assert rel_err(PHI - 1.0, want) <= k * k * EPS * Lk + 2 * EPS / np.abs(want).max()
    dev = torch.device("cuda")
    D = torch.ones(N * N, dtype=torch.float64, device=dev)
    t = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(dev)      # noqa: E731
    dm, dg, dic = t(mk), t(g.ravel()), t(ic)
    _lib.check(_lib.lib().bluest_objectiveK_f64(D.data_ptr(), N, k, Lk, dm.data_ptr(), dg.data_ptr(), dic.data_ptr()))
    assert rel_err(D.cpu().numpy() - 1.0, want) <= k * k * EPS * Lk + 2 * EPS / np.abs(want).max()
    grad = torch.full((Lk,), 2.0, dtype=torch.float64, device=dev)
    v = t(P[0])
    _lib.check(_lib.lib().bluest_gradK(grad.data_ptr(), k, Lk, dg.data_ptr(), dic.data_ptr(), v.data_ptr(), N))
    gw = oracle.gradK(k, Lk, g, ic, P)
    assert rel_err(grad.cpu().numpy() - 2.0, gw) <= 10 * k * k * EPS + 4 * EPS / np.abs(gw).max()


def test_objectiveK_grid_stride_beyond_1024_workgroups(gpu, oracle):
    """Lk > 262 144 = 1024 workgroups x 256 threads: the grid-stride loop of k_objectiveK takes more than one round"""
    from bluest_amd import misc
    rng = np.random.RandomState(3)
    N, k, Lk = 20, 2, 300000
    g = _rand_groups(N, k, 1000, rng)[rng.randint(0, 1000, Lk)]
    ic = (np.repeat(_rand_inv(k, 1, rng)[None], Lk, axis=0) * (0.5 + rng.rand(Lk))[:, None]).reshape(-1)
    mk = 0.5 + rng.rand(Lk)
    got = misc.objectiveK(N, k, Lk, mk, g, ic)
    want = oracle.objectiveK(N, k, Lk, mk, g, ic)
    # an entry sums up to Lk products: Lk eps sum|t|, relative to the largest entry
    absum = oracle.objectiveK(N, k, Lk, mk, g, np.abs(ic))
    bound = Lk * EPS * np.abs(absum).max() / np.abs(want).max()
    assert rel_err(got, want) <= min(bound, 1e-10)


def test_variance_GH_hessian_on_wide_groups(gpu, oracle):
    """SAP.variance_GH with the Hessian (hessKQ for every (k, q) pair) on a plan of 17- and 32-model groups, against OracleSAP"""
    from bluest_amd.sap import SAP
    rng = np.random.RandomState(5)
    N, K = 32, 32
    C = synth.wishart_covariance(N, 0)[0]
    groups = [np.arange(N).reshape(-1, 1)]
    for k in range(2, K + 1):
        cnt = {2: 30, 17: 6, 32: 1}.get(k, 0)
        groups.append(_rand_groups(N, k, cnt, rng) if cnt else np.zeros((0, k), dtype=np.int64))
    costs = np.concatenate([np.full(len(g), 1.0 + k) for k, g in enumerate(groups)])
    sap = SAP(C.copy(), K, [g.copy() for g in groups], costs, verbose=False)
    ref = oracle.OracleSAP(C.copy(), K, [g.copy() for g in groups], costs)
    m = 0.5 + rng.rand(len(costs))
    V, g, H = sap.variance_GH(m)
    Vr, gr, Hr = ref.variance_GH(m)
    assert abs(V / Vr - 1) < 1e-11 and rel_err(g, gr) < 1e-11
    assert rel_err(H, Hr) < 1e-10                        # the bar of the golden Hessians (test_gpu_parity._check_sap_file)

"""
GPU tests (-m gpu) of model groups wider than 16 models (up to BLUEST_MAX_GROUP = 32): the wide-group pseudo-inverse
(k_group_pinv_wide), evaluation of plans holding such groups against the CPU oracle, the second-order solve with wide groups
in the support, phase 1 on single-output plans of 13..16-model groups, and the BLUEProblem front end at 18 models.
"""
import numpy as np
import pytest

from conftest import rel_err

pytestmark = pytest.mark.gpu

EPS = np.finfo(np.float64).eps


@pytest.fixture(scope="module")
def gpu():
    import torch
    from bluest_amd import _lib
    assert torch.cuda.is_available(), "these tests need the MI355X"
    assert _lib.device_count() >= 1
    return torch


def _wishart(n, seed, dof=None):
    rng = np.random.RandomState(seed)
    A = rng.randn(n, dof or 4 * n)
    return A @ A.T / (dof or 4 * n), rng


def _correlated(n, seed, rho=0.95):
    """multifidelity-like covariance: every model strongly correlated with model 0 and with its neighbours"""
    rng = np.random.RandomState(seed)
    idx = np.arange(n)
    S = rho ** np.abs(idx[:, None] - idx[None, :])
    A = np.linalg.cholesky(S) @ rng.randn(n, 6 * n)
    C = A @ A.T / (6 * n)
    d = 1.0 / np.sqrt(np.diag(C))
    return C * d[:, None] * d[None, :], rng


def _levels(groups, K):
    """list over k = 1..K of (L_k, k) int64 arrays from a list of model tuples (sorted, lexicographic per size)"""
    out = []
    for k in range(1, K + 1):
        gk = sorted(tuple(sorted(int(i) for i in g)) for g in groups if len(g) == k)
        out.append(np.array(gk, dtype=np.int64).reshape(-1, k))
    return out


def _pinv_ref(C, g):
    sub = C[np.ix_(g, g)]
    return np.linalg.pinv(0.5 * (sub + sub.T))


# ---- the pseudo-inverse of wide groups ----------------------------------------------------------------------------------------

@pytest.mark.parametrize("k", [17, 20, 24, 31, 32])
def test_group_pinv_wide_vs_numpy(gpu, oracle, k):
    """bluest_group_pinv (int64 groups) and the plan's set-up (uint8 device copy of the groups) against numpy.linalg.pinv on
    Wishart blocks (1e-12), rank-deficient blocks (one model duplicated) and blocks of condition ~1e8 (100 cond eps)"""
    from bluest_amd import misc
    from bluest_amd.plan import Plan
    n = 40
    C, rng = _wishart(n, 100 + k)
    # a duplicated model: 39 is a copy of 1
    Cd = C.copy()
    Cd[39, :] = Cd[1, :]
    Cd[:, 39] = Cd[:, 1]
    Cd[39, 39] = Cd[1, 1]
    # condition ~1e8
    Q, _ = np.linalg.qr(rng.randn(n, n))
    Cc = (Q * np.logspace(0, -8, n)) @ Q.T
    groups = [np.sort(rng.choice(n, k, replace=False)) for _ in range(5)]
    groups.append(np.arange(k))
    groups_d = [np.sort(np.concatenate([[1, 39], rng.choice(np.arange(2, 39), k - 2, replace=False)])) for _ in range(3)]
    for Cx, gl, kind in ((C, groups, "wishart"), (Cd, groups_d, "rank-deficient"), (Cc, groups, "cond 1e8")):
        g = np.ascontiguousarray(np.array(gl, dtype=np.int64))
        got_i64 = misc.group_pinv(Cx, k, g).reshape(len(gl), k, k)
        sizes = [0] * (k - 1) + [len(gl)]
        plan = Plan(n, len(gl), [{"K": k, "sizes": sizes, "groups": [np.zeros((0, j), dtype=np.int64) for j in range(1, k)] + [g],
                                  "C": Cx, "mapping": None}])
        got_u8 = np.asarray(plan.invcovs[0]).reshape(len(gl), k, k)
        ref_c = oracle.c_group_pinv(Cx, k, g).reshape(len(gl), k, k)
        for i, gi in enumerate(gl):
            want = _pinv_ref(Cx, gi)
            w = np.abs(np.linalg.eigvalsh(0.5 * (Cx[np.ix_(gi, gi)] + Cx[np.ix_(gi, gi)].T)))
            cond = w.max() / w[w > 1e-15 * w.max()].min()
            tol = 1e-12 if kind == "wishart" else 100 * cond * EPS
            for got, path in ((got_i64[i], "int64"), (got_u8[i], "uint8")):
                err = np.linalg.norm(got - want) / np.linalg.norm(want)
                assert err <= tol, (k, kind, path, i, err, tol)
            assert np.linalg.norm(ref_c[i] - want) / np.linalg.norm(want) <= max(tol, 1e-12), (k, kind, "oracle")


def test_group_pinv_wide_scaled_norm(gpu):
    """pinv(2^515 C) == 2^-515 pinv(C), bit for bit, on both paths (int64 groups of bluest_group_pinv, uint8 groups of the plan's
    set-up).  The entries of 2^515 C are near 1e155: a plain sum of their squares is inf, and with it the rotation tolerance, so
    no rotation would be taken and diag(1 / a_ii) returned as a converged result; the norm is formed from entries scaled by the
    largest.  Every operation of the routine commutes with a power-of-two scale (the rotation angles come from the scale-free
    tau, the cut-off is relative, nothing underflows or overflows at these magnitudes), hence equality rather than a tolerance."""
    from bluest_amd import misc
    from bluest_amd.plan import Plan
    n = 32
    C, rng = _wishart(n, 515)
    scale = 2.0 ** 515
    with np.errstate(over="ignore"):
        assert np.isinf(((scale * C[:17, :17]) ** 2).sum()) and np.isfinite(scale * C).all()
    for k, gl in ((17, [np.sort(rng.choice(n, 17, replace=False)) for _ in range(2)]), (32, [np.arange(32), np.arange(32)])):
        g = np.ascontiguousarray(np.array(gl, dtype=np.int64))
        sizes = [0] * (k - 1) + [len(gl)]

        def both(Cx):
            plan = Plan(n, len(gl), [{"K": k, "sizes": sizes, "groups": [np.zeros((0, j), dtype=np.int64) for j in range(1, k)] + [g],
                                      "C": Cx, "mapping": None}])
            return (misc.group_pinv(Cx, k, g).reshape(len(gl), k, k), np.asarray(plan.invcovs[0]).reshape(len(gl), k, k).copy())
        for path, small, big in zip(("int64", "uint8"), both(C), both(scale * C)):
            want = small / scale                                  # exact: a power of two, far from the subnormals
            assert np.isfinite(big).all() and np.abs(want).min() > 1e-200, (k, path)
            for i, gi in enumerate(gl):                           # the unscaled side is a pseudo-inverse at all
                ref = _pinv_ref(C, gi)
                assert np.linalg.norm(small[i] - ref) / np.linalg.norm(ref) <= 1e-12, (k, path, i)
            print("k=%d %s: %d of %d entries differ" % (k, path, int((big != want).sum()), big.size))
            assert np.array_equal(big, want), (k, path)


def test_group_size_limit_is_enforced(gpu):
    """33 models in one group: refused with BLUEST_ERR_ARG and a message naming the limit (plan and mirror alike)"""
    from bluest_amd import misc
    from bluest_amd._lib import BluestHipError
    from bluest_amd.sap import SAP
    n = 40
    C, _ = _wishart(n, 7)
    g = np.arange(33, dtype=np.int64)[None, :]
    with pytest.raises(BluestHipError, match="32"):
        misc.group_pinv(C, 33, g)
    groups = _levels([(i,) for i in range(n)] + [tuple(range(33))], 33)
    with pytest.raises(BluestHipError, match="BLUEST_MAX_GROUP = 32"):
        SAP(C, 33, groups, np.ones(n + 1), verbose=False)


# ---- evaluation ---------------------------------------------------------------------------------------------------------------

def _wide_group_list(n, rng, sizes):
    gl = [(i,) for i in range(n)] + [tuple(sorted(rng.choice(n, 2, replace=False))) for _ in range(30)]
    gl += [tuple(sorted(rng.choice(n, 3, replace=False))) for _ in range(20)]
    for k in sizes:
        gl += [tuple(sorted(rng.choice(n, k, replace=False))) for _ in range(2)]
    gl.append(tuple(range(32)))
    return sorted(set(gl), key=lambda g: (len(g), g))


def _tol(oracle_sap, m):
    cond = np.linalg.cond(oracle_sap.get_phi(m))
    return 1e-11 if cond * EPS < 1e-13 else 1e-9


def test_sap_evaluation_wide_groups_vs_oracle(gpu, oracle):
    """SAP at n = 40 with groups of 1, 2, 3 and 17..32 models (some size buckets empty, arange(32) included): variance,
    variance_GH(nohess=True) and get_phi against OracleSAP"""
    from bluest_amd.sap import SAP
    n, K = 40, 32
    C, rng = _wishart(n, 11)
    sizes = [17, 18, 20, 23, 24, 27, 29, 31]            # 19, 21, 22, 25, 26, 28, 30 (and 4..16) stay empty
    gl = _wide_group_list(n, rng, sizes)
    levels = _levels(gl, K)
    w = 1.0 + rng.rand(n)
    costs = np.concatenate([w[lv].sum(axis=1) if len(lv) else np.zeros(0) for lv in levels])
    sap = SAP(C, K, [lv.copy() for lv in levels], costs, verbose=False)
    ref = oracle.OracleSAP(C, K, [lv.copy() for lv in levels], costs)
    for trial in range(3):
        m = 0.5 + 10.0 * rng.rand(len(costs))
        tol = _tol(ref, m)
        assert abs(sap.variance(m) / ref.variance(m) - 1) <= tol
        V, g, _ = sap.variance_GH(m, nohess=True)
        Vr, gr, _ = ref.variance_GH(m, nohess=True)
        assert abs(V / Vr - 1) <= tol and rel_err(g, gr) <= tol, (trial, rel_err(g, gr))
        assert rel_err(sap.get_phi(m), ref.get_phi(m)) <= tol


def test_mosap_evaluation_wide_groups_vs_oracle(gpu, oracle):
    """3-output MOSAP whose outputs have different group sets, wide groups in each"""
    from bluest_amd.mosap import MOSAP
    n, K, n_out = 40, 32, 3
    rng = np.random.RandomState(5)
    Cs = [_wishart(n, 20 + o)[0] for o in range(n_out)]
    per_out = [_wide_group_list(n, np.random.RandomState(30 + o), [17 + 3 * o, 24 + o, 31 - o]) for o in range(n_out)]
    union = sorted(set(g for gl in per_out for g in gl), key=lambda g: (len(g), g))
    w = 1.0 + rng.rand(n)
    groups = _levels(union, K)
    multi_groups = [_levels(gl, K) for gl in per_out]
    gc = lambda lv: np.concatenate([w[x].sum(axis=1) if len(x) else np.zeros(0) for x in lv])
    mos = MOSAP(Cs, K, [K] * n_out, [x.copy() for x in groups], [[x.copy() for x in mg] for mg in multi_groups], gc(groups),
                [gc(mg) for mg in multi_groups], verbose=False)
    ref = oracle.OracleMOSAP(Cs, K, [K] * n_out, [x.copy() for x in groups], [[x.copy() for x in mg] for mg in multi_groups],
                             gc(groups), [gc(mg) for mg in multi_groups])
    m = 0.5 + 10.0 * rng.rand(len(union))
    Vs = np.asarray(mos.variances(m))
    Vr = np.asarray(ref.variances(m))
    tol = max(_tol(oracle.OracleSAP(Cs[o], K, [x.copy() for x in multi_groups[o]], gc(multi_groups[o])), m[mos.mappings[o]])
              for o in range(n_out))
    assert rel_err(Vs, Vr) <= tol
    Vg, grads, _ = mos.variance_GH(m, nohess=True)
    Vgr, gradsr, _ = ref.variance_GH(m, nohess=True)
    assert rel_err(Vg, Vgr) <= tol
    for o in range(n_out):
        assert rel_err(grads[o], gradsr[o]) <= tol, o


def test_group_sharded_plans_wide_groups(gpu, oracle):
    """the group-sharded evaluation (shard plans: Phi records, record solve, shard gradients) over a plan with wide groups
    equals the unsharded one and the oracle's Phi, with 2 shards on one GPU"""
    import test_gpu_parity as tp
    from bluest_amd.plan import Plan
    torch = gpu
    n, K = 40, 32
    C, rng = _wishart(n, 12)
    gl = _wide_group_list(n, rng, [17, 21, 26, 32 - 1])
    levels = _levels(gl, K)
    sizes = [len(x) for x in levels]
    outs = [{"K": K, "sizes": sizes, "groups": levels, "C": C, "mapping": None}]
    full = Plan(n, len(gl), outs)
    mappings = [np.arange(len(gl), dtype=np.int64)]
    m_h = 0.5 + 10.0 * rng.rand(len(gl))
    m = torch.from_numpy(m_h).to(full.device)
    ref = oracle.OracleSAP(C, K, [x.copy() for x in levels], np.ones(len(gl)))
    tp._check_shards_against_full(torch, n, sizes, outs, full, mappings, m, (2,), phi_oracle=ref.get_phi(m_h))


# ---- solves -------------------------------------------------------------------------------------------------------------------

def _factor(n, seed):
    """one-factor covariance: every model is model 0's signal plus its own noise (cheap, individually poor models whose
    combination pays: the optimal allocation couples many of them in one group)"""
    rng = np.random.RandomState(seed)
    d = np.concatenate([[0.01], rng.uniform(0.5, 2.0, n - 1)])
    return np.ones((n, n)) + np.diag(d), rng


def _solve_problem(n, seed, n_wide=40, wide=(17, 24), full=True):
    C, rng = _factor(n, seed)
    w = np.concatenate([[1.0], 10.0 ** -rng.uniform(2.0, 3.0, n - 1)])
    gl = [(i,) for i in range(n)] + [(i, j) for i in range(n) for j in range(i + 1, n)]
    wide_g = set()
    while len(wide_g) < n_wide:
        k = rng.randint(wide[0], wide[1] + 1)
        wide_g.add(tuple(sorted(rng.choice(n, k, replace=False))))
    gl += sorted(wide_g)
    if full:
        gl.append(tuple(range(n)))
    return C, w, sorted(set(gl), key=lambda g: (len(g), g))


def _sap(C, w, gl):
    from bluest_amd.sap import SAP
    K = max(len(g) for g in gl)
    levels = _levels(gl, K)
    costs = np.concatenate([w[x].sum(axis=1) if len(x) else np.zeros(0) for x in levels])
    return SAP(C, K, [x.copy() for x in levels], costs, verbose=False), levels, costs, K


def _certify(oracle, C, K, levels, costs, m, s=None):
    sap = oracle.SparseOracleSAP(C, K, [x.copy() for x in levels])
    gap, lb, mu, info = oracle.optimality_certificate([sap], m, costs, s=s, max_seconds=150)
    return gap, sap.variance(m)


@pytest.mark.parametrize("mode", ["budget", "eps"])
def test_sap_solve_with_wide_groups_is_certified(gpu, oracle, mode):
    """n = 24: all singletons, all pairs, 40 random groups of 17..24 models and the full group.  Certified by the oracle's own
    dual, second-order path, no worse than without the wide groups, and (over the cases) a wide group in the optimal support"""
    n = 24
    wide_used = []
    for seed in (1, 2):
        C, w, gl = _solve_problem(n, seed)
        sap, levels, costs, K = _sap(C, w, gl)
        narrow = [g for g in gl if len(g) <= 2]
        sap0, levels0, costs0, K0 = _sap(C, w, narrow)
        if mode == "budget":
            B = 50.0 * w.sum()
            m = sap.solve(budget=B, continuous_relaxation=True)
            m0 = sap0.solve(budget=B, continuous_relaxation=True)
            assert m is not None and abs(m @ costs / B - 1) < 1e-9
            assert sap.variance(m) <= sap0.variance(m0) * (1 + 1e-9)
            gap, _ = _certify(oracle, C, K, levels, costs, m)
        else:
            eps = float(np.sqrt(C[0, 0]) / 100.0)
            m = sap.solve(eps=eps, continuous_relaxation=True)
            m0 = sap0.solve(eps=eps, continuous_relaxation=True)
            assert m is not None and sap.variance(m) <= eps ** 2 * (1 + 1e-9)
            assert m @ costs <= (m0 @ costs0) * (1 + 1e-9)
            gap, _ = _certify(oracle, C, K, levels, costs, m, s=np.array([eps ** 2]))
        info = sap.solver_info
        print("wide solve %s seed %d: gap %.3e, solver gap %.3e, support %d, wide in support %d" % (
            mode, seed, gap, info.get("certified_gap", np.nan), int((m > 0).sum()), int((m[-n_wide_count(levels):] > 0).sum())))
        assert info.get("method") == "newton", info
        assert gap <= 1e-8, (mode, seed, gap)
        wide_used.append(int((m[-n_wide_count(levels):] > 0).sum()))
    assert max(wide_used) > 0, wide_used


def n_wide_count(levels):
    return sum(len(x) for x in levels[16:])


def test_sap_solve_wide_groups_integer_and_caps(gpu, oracle):
    """the same problem with the integer projection (continuous_relaxation=False) and with per-model sample caps.  The continuous
    uncapped optimum bounds both from below; both are no worse than the same solve without the wide groups; the capped solve
    carries its own certificate (Lagrangian relaxation of the caps)"""
    n = 24
    C, w, gl = _solve_problem(n, 3)
    sap, levels, costs, K = _sap(C, w, gl)
    narrow = [g for g in gl if len(g) <= 2]
    sap0, levels0, costs0, K0 = _sap(C, w, narrow)
    B = 50.0 * w.sum()
    mc = sap.solve(budget=B, continuous_relaxation=True)
    Vc = sap.variance(mc)
    mi = sap.solve(budget=B)
    assert mi is not None and (mi == np.round(mi)).all() and mi @ costs <= B * (1 + 1e-12)
    assert sap.solver_info.get("method") == "newton", sap.solver_info
    Vi = sap.variance(mi)
    mi0 = sap0.solve(budget=B)
    print("integer: V %.6e, continuous optimum %.6e, without wide groups %.6e" % (Vi, Vc, sap0.variance(mi0)))
    assert Vc * (1 - 1e-9) <= Vi <= 1.1 * Vc
    assert Vi <= sap0.variance(mi0) * (1 + 1e-9)
    caps = np.full(n, np.inf)
    allg = [tuple(x) for lv in levels for x in lv]
    used = np.array([sum(mc[i] for i, g in enumerate(allg) if j in g) for j in range(n)])
    j = 1 + int(np.argmax(used[1:]))
    caps[j] = 0.5 * used[j]
    mcap = sap.solve(budget=B, continuous_relaxation=True, max_model_samples=caps)
    assert mcap is not None
    assert sum(mcap[i] for i, g in enumerate(allg) if j in g) <= caps[j] * (1 + 1e-9)
    info = sap.solver_info
    assert info.get("method") == "newton", info
    Vcap = sap.variance(mcap)
    mcap0 = sap0.solve(budget=B, continuous_relaxation=True, max_model_samples=caps)
    print("capped: V %.6e, uncapped optimum %.6e, without wide groups %.6e, solver gap %.3e" % (
        Vcap, Vc, sap0.variance(mcap0), info.get("certified_gap", np.nan)))
    assert Vcap >= Vc * (1 - 1e-9)
    assert Vcap <= sap0.variance(mcap0) * (1 + 1e-9)
    assert info["certified_gap"] <= 1e-6, info["certified_gap"]       # 9.8e-8 measured: the caps enter by Lagrangian relaxation


def test_sharded_two_ranks_wide_groups(gpu, tmp_path):
    """two ranks (two processes on the one GPU, gloo) over group sets with groups of 17..24 models (on both shards):
    the sharded evaluation equals the single-process plan, and the sharded solve reaches the single-GPU optimum with a
    certified gap, identical on both ranks, with a wide group in its support"""
    import json
    import os
    import subprocess
    import sys
    from conftest import ROOT
    out = str(tmp_path / "wide_sharded.json")
    env = dict(os.environ, MASTER_ADDR="127.0.0.1")
    cmd = [sys.executable, "-m", "torch.distributed.run", "--nnodes=1", "--nproc-per-node", "2", "--master-addr", "127.0.0.1",
           "--master-port", "29541", os.path.join(ROOT, "tests", "wide_sharded_worker.py"), out]
    proc = subprocess.run(cmd, env=env, capture_output=True, text=True, timeout=600)
    assert proc.returncode == 0, proc.stdout[-3000:] + proc.stderr[-3000:]
    res = json.load(open(out))
    print(res)
    assert res["world"] == 2
    for tag in ("n24_o1", "n20_o2"):
        assert res[tag + "_eval_err"] < 1e-12 and res[tag + "_grad_err"] < 1e-12 and res[tag + "_status_equal"], tag
        lo, hi = res[tag + "_shard"]
        assert lo == 0 and res[tag + "_wide_first"] < hi < res[tag + "_L"], (tag, lo, hi)      # wide groups on both shards
        assert res[tag + "_ranks_agree"] and abs(res[tag + "_cost_ratio"] - 1) < 1e-9
        assert res[tag + "_method"] == "newton" and res[tag + "_gap"] <= 1e-8, (tag, res[tag + "_method"], res[tag + "_gap"])
        assert abs(res[tag + "_F_sharded"] / res[tag + "_F_single"] - 1) < 1e-8, tag
        assert res[tag + "_wide_in_support"] > 0, tag


def test_sap_solve_groups_13_to_16(gpu):
    """single-output solves on plans whose widest group has 13..16 models: phase 1 runs evaluate + bluest_ma_update (the fused
    multiplicative tail stops at 12) and the solve ends certified"""
    from bluest_amd.plan import Plan
    n = 16
    C, rng = _factor(n, 9)
    w = np.concatenate([[1.0], 10.0 ** -rng.uniform(2.0, 3.0, n - 1)])
    for kw in (13, 16):
        gl = [(i,) for i in range(n)] + [(i, j) for i in range(n) for j in range(i + 1, n)]
        gl += [tuple(sorted(rng.choice(n, k, replace=False))) for k in range(13, kw + 1) for _ in range(3)]
        gl = sorted(set(gl), key=lambda g: (len(g), g))
        sap, levels, costs, K = _sap(C, w, gl)
        m = sap.solve(budget=50.0 * w.sum(), continuous_relaxation=True)
        assert m is not None, kw
        assert sap.solver_info.get("method") == "newton", sap.solver_info
        assert sap.solver_info["certified_gap"] <= 1e-8, sap.solver_info["certified_gap"]


# ---- front end ----------------------------------------------------------------------------------------------------------------

def test_blueproblem_K_equals_18_models(gpu):
    """BLUEProblem(18, C, costs).setup_solver(K=18): 262 143 groups, wide ones included; meets eps at a total cost no higher
    than with K=16, and solve() samples the allocation"""
    from bluest_amd import BLUEProblem
    n = 18
    C, rng = _correlated(n, 4)
    costs = np.concatenate([[1.0], 10.0 ** -rng.uniform(1.0, 3.0, n - 1)])

    class P(BLUEProblem):
        def sampler(self, ls):
            z = rng.randn()
            return [z for _ in ls]

        def evaluate(self, ls, samples):
            return [[samples[i] * (1.0 + 0.01 * ls[i]) for i in range(len(ls))]]     # outputs x models

    p = P(n, C=C.copy(), costs=costs, verbose=False)
    eps = float(np.sqrt(C[0, 0]) / 50.0)
    d16 = p.setup_solver(K=16, eps=eps, continuous_relaxation=True)
    d18 = p.setup_solver(K=18, eps=eps, continuous_relaxation=True)
    assert d18["errors"][0] <= eps * (1 + 1e-6)
    assert d18["total_cost"] <= d16["total_cost"] * (1 + 1e-9), (d18["total_cost"], d16["total_cost"])
    p18 = P(n, C=C.copy(), costs=costs, verbose=False)
    d = p18.setup_solver(K=18, eps=eps)
    assert (d["samples"] > 0).all() and d["errors"][0] <= eps * 1.0001
    mus, errs, tot = p18.solve(K=18, eps=eps)
    assert np.isfinite(mus[0]) and tot == d["total_cost"]


def test_blueproblem_refuses_a_33_model_group(gpu):
    from bluest_amd import BLUEProblem
    from bluest_amd._lib import BluestHipError
    n = 40
    C, _ = _wishart(n, 3)
    p = BLUEProblem(n, C=C, costs=np.ones(n), verbose=False)
    groups = [[i] for i in range(n)] + [list(range(33))]
    with pytest.raises(BluestHipError, match="BLUEST_MAX_GROUP = 32"):
        p.setup_solver(groups=groups, budget=100.0)

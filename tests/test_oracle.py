"""
CPU tests (-m "not gpu"): pin the oracle (oracle/oracle.py + oracle/bluest_oracle.c) against the golden vectors
produced by the real reference (oracle/gen_golden.py).  Tolerance: 1e-13 relative on the numpy
restatement; 1e-9..1e-11 on the pure-C Jacobi/LU twins for quantities that go through a pseudo-inverse of an
ill-conditioned matrix (documented per test).
"""
import numpy as np
import pytest

from bluest_amd import synth
from conftest import golden, rel_err


def _split(prefix, G):
    return {k[len(prefix):]: v for k, v in G.items() if k.startswith(prefix)}


def test_cmisc_known_answers(oracle):
    """every native function of cmisc.cpp:99-110 against the compiled reference's outputs"""
    G = golden("cmisc_known_answers.npz")
    N = int(G["N"])
    for k, q in ((1, 2), (2, 3), (3, 3), (4, 2)):
        g = _split("k%dq%d_" % (k, q), G)
        Lk, Lq = len(g["gk"]), len(g["gq"])
        assert rel_err(oracle.assemble_psi(N, k, Lk, g["gk"], g["ick"]), g["psi"]) == 0.0
        assert rel_err(oracle.objectiveK(N, k, Lk, g["mk"], g["gk"], g["ick"]), g["PHI"]) < 1e-15
        assert rel_err(oracle.objectiveK(N, k, Lk, g["mki"], g["gk"], g["ick"]), g["PHIi"]) < 1e-15
        assert rel_err(oracle.gradK(k, Lk, g["gk"], g["ick"], g["P"]), g["grad"]) < 1e-14
        assert rel_err(oracle.cleanupK(k, Lk, g["gk"], g["ick"], g["P"]), g["X"]) < 1e-15
        assert rel_err(oracle.hessKQ(k, q, Lk, Lq, g["gk"], g["gq"], g["ick"], g["icq"], g["P"]), g["hess"]) < 1e-13


CASES = ("base", "sparse", "drop_last_model", "only_first3", "int64")


def _check_sap_file(oracle, fname, tol=1e-13):
    G = golden(fname)
    n, kmax, n_out = int(G["n"]), int(G["kmax"]), int(G["n_out"])
    prob = synth.problem(n, kmax, n_out)
    for o in range(n_out):
        sap = oracle.OracleSAP(prob["C"][o], kmax, prob["groups"], prob["costs"])
        if o == 0:
            ic = np.concatenate(sap.invcovs)
            if "invcovs_o0" in G:
                assert rel_err(ic, G["invcovs_o0"]) < 1e-14
            else:
                assert rel_err(ic[::101], G["invcovs_o0_sub"]) < 1e-14
                assert abs(np.linalg.norm(ic) / G["invcovs_o0_norm"] - 1) < 1e-14
            if "psi_o0" in G:
                assert rel_err(sap.psi, G["psi_o0"]) < 1e-14
        for name in CASES:
            m = prob["m"][o] if name == "base" else G["o%d_%s_m" % (o, name)]
            mf = m.astype(np.float64)
            for delta in ((0.0, 1e-6) if name in ("base", "drop_last_model") else (0.0,)):
                tag = "o%d_%s_" % (o, name) + ("d%g_" % delta if delta else "")
                assert abs(sap.variance(mf, delta=delta) / G[tag + "V"] - 1) < tol
                V, grad, _ = sap.variance_GH(mf, delta=delta, nohess=True)
                assert abs(V / G[tag + "Vgh"] - 1) < tol
                assert rel_err(sap.get_phi(mf, delta=delta), G[tag + "PHI"]) < tol
                if tag + "grad" in G:
                    assert rel_err(grad, G[tag + "grad"]) < tol
                else:
                    assert rel_err(grad[::97], G[tag + "grad_sub"]) < tol
                    assert abs(np.linalg.norm(grad) / G[tag + "grad_norm"] - 1) < tol
                if tag + "hess" in G:
                    assert rel_err(sap.variance_GH(mf, delta=delta)[2], G[tag + "hess"]) < 1e-12
        # all-tiny allocation -> inf (misc.py:464,484)
        assert np.isinf(sap.variance(0.01 * np.ones(sap.L))) and np.isinf(G["o%d_tiny_V" % o])
        Vt, gt = sap.variance_GH(0.01 * np.ones(sap.L), nohess=True)[:2]
        assert np.isinf(Vt) and np.isinf(gt).all() and bool(G["o%d_tiny_grad_isinf" % o])
        # int64 allocation through the sparse native loop (cmisc.cpp:105) == dense psi@m
        mi = G["o%d_int64_m" % o]
        PHI = np.zeros(n * n)
        for k in range(1, kmax + 1):
            PHI += oracle.objectiveK(n, k, sap.sizes[k], mi[sap.cumsizes[k - 1]:sap.cumsizes[k]],
                                     sap.groups[k - 1], sap.invcovs[k - 1])
        assert rel_err(PHI.reshape(n, n), G["o%d_int64_PHI_native" % o]) < 1e-14


@pytest.mark.parametrize("fname", ["sap_n5_all.npz", "sap_n6_all.npz", "sap_n12_all.npz"])
def test_sap_small(oracle, fname):
    _check_sap_file(oracle, fname)


def test_sap_n20_k5_o8(oracle):
    _check_sap_file(oracle, "sap_n20_k5_o8.npz")


def test_model0_unsampled_asserts(oracle):
    """misc.py:470: variance() raises AssertionError when no sampled group contains model 0"""
    prob = synth.problem(5, 3, 1)
    sap = oracle.OracleSAP(prob["C"][0], 3, prob["groups"], prob["costs"])
    m = prob["m"][0].copy()
    m[sap.e == 1] = 0.0
    with pytest.raises(AssertionError):
        sap.variance(m)
    rc, _ = sap.c_variance(m)
    assert rc == 2


def test_pure_c_twins(oracle):
    """the plain-C evaluation (Jacobi pinv / LU solve, no LAPACK) agrees with the numpy restatement; this is the
    code timed as bench.py's cpu_baseline"""
    for n, kmax in ((6, 6), (12, 5)):
        prob = synth.problem(n, kmax, 1)
        sap = oracle.OracleSAP(prob["C"][0], kmax, prob["groups"], prob["costs"])
        m = prob["m"][0]
        for dense in (False, True):
            rc, V = sap.c_variance(m, dense=dense)
            assert rc == 0 and abs(V / sap.variance(m) - 1) < 1e-11
            rc, V, grad, v, PHI = sap.c_variance_GH(m, dense=dense)
            Vr, gr, _ = sap.variance_GH(m, nohess=True)
            assert rc == 0 and abs(V / Vr - 1) < 1e-10
            assert rel_err(grad, gr) < 1e-10
            assert rel_err(PHI, sap.get_phi(m)) < 1e-14
        for k in (1, 2, 3, kmax):
            assert rel_err(oracle.c_group_pinv(prob["C"][0], k, sap.groups[k - 1]), sap.invcovs[k - 1]) < 1e-11


def test_mosap_ragged(oracle):
    """multi-output with different group sets per output (mosap.py:54-67 mappings, :86-100 fan-out)"""
    G = golden("mosap_n6_o3_ragged.npz")
    n, n_out, kmax = int(G["n"]), int(G["n_out"]), int(G["kmax"])
    prob = synth.problem(n, kmax, n_out)
    groups = [G["g_k%d" % k] for k in range(1, kmax + 1)]
    multi_groups = [[G["mg%d_k%d" % (o, k)] for k in range(1, kmax + 1)] for o in range(n_out)]
    w = prob["w"]
    mos = oracle.OracleMOSAP(prob["C"], kmax, [kmax] * n_out, groups, multi_groups, synth.group_costs(groups, w),
                             [synth.group_costs(mg, w) for mg in multi_groups])
    for o in range(n_out):
        assert (mos.mappings[o] == G["map%d" % o]).all()
    assert (mos.e == G["e"]).all()
    assert rel_err(mos.variances(G["m"]), G["Vs"]) < 1e-13
    Vgh, grads, _ = mos.variance_GH(G["m"], nohess=True)
    assert rel_err(Vgh, G["Vgh"]) < 1e-13
    for o in range(n_out):
        assert rel_err(grads[o], G["grad%d" % o]) < 1e-13


def test_hh_paper_known_answer(oracle):
    """Hodgkin-Huxley paper fixture: stored allocation -> errors/eps and total cost.
    cond(C) is 1e9..5e10 here, so V is compared at 1e-6 (pinv of ill-conditioned blocks), the cost exactly."""
    G = golden("hh_paper_known_answer.npz")
    n, n_out, kmax = int(G["n"]), int(G["n_out"]), int(G["kmax"])
    groups = synth.all_groups(n, kmax)
    costs = synth.group_costs(groups, G["costs"])
    Cs = [G["C%d" % o] for o in range(n_out)]
    mos = oracle.OracleMOSAP(Cs, kmax, [kmax] * n_out, groups, [groups] * n_out, costs, [costs] * n_out)
    samples = G["samples"]
    Vs = np.array(mos.variances(samples.astype(np.float64)))
    assert rel_err(Vs, G["Vs"]) < 1e-6
    eps = np.sqrt(np.array([C[0, 0] for C in Cs])) / 1000
    assert np.allclose(np.sqrt(Vs) / eps, [0.8906, 1.00004, 0.9479, 0.5477, 0.5583], rtol=2e-4)
    assert abs(float(samples @ costs) - float(G["total_cost"])) < 1e-9 * float(G["total_cost"])
    assert abs(float(G["total_cost"]) - 60626.8057) < 1e-3


def _ns_case(G, case):
    n_out, kmax = int(G["n_out"]), int(G["kmax"])
    groups = [G["%s_g_k%d" % (case, k)] for k in range(1, kmax + 1)]
    maps = [G["%s_map%d" % (case, o)] for o in range(n_out)]
    flat = np.concatenate([np.pad(g, ((0, 0), (0, kmax - g.shape[1])), constant_values=-1) for g in groups])
    cum = np.cumsum([0] + [len(g) for g in groups])
    multi = []
    for o in range(n_out):                       # output o's own group lists, recovered through its mapping
        rows = flat[maps[o]]
        multi.append([rows[(maps[o] >= cum[k]) & (maps[o] < cum[k + 1]), :k + 1] for k in range(kmax)])
    return groups, maps, multi


@pytest.mark.parametrize("case", ["full", "ragged"])
def test_ns_paper_known_answer(oracle, case):
    """Navier-Stokes paper data (bluest_NS.py:115-142): 12 models, 6 outputs, K = 7, cond(Phi) up to 1.8e10; `ragged` = every
    output on its own ~60 % of the groups.  The restatement reproduces the reference's mappings exactly and V / grad V to
    cond * eps."""
    G = golden("ns_paper_known_answer.npz")
    n_out, kmax = int(G["n_out"]), int(G["kmax"])
    groups, maps, multi = _ns_case(G, case)
    Cs = [G["C%d" % o] for o in range(n_out)]
    costs = synth.group_costs(groups, G["costs"])
    assert rel_err(costs, G["%s_group_costs" % case]) < 1e-15
    mos = oracle.OracleMOSAP(Cs, kmax, [kmax] * n_out, groups, multi, costs, [synth.group_costs(mg, G["costs"]) for mg in multi])
    assert mos.L == int(G["%s_L" % case])
    for o in range(n_out):
        assert np.array_equal(mos.mappings[o], maps[o])
    for tag in ("dense", "sparse"):
        m = G["%s_m_%s" % (case, tag)]
        assert rel_err(mos.variances(m), G["%s_Vs_%s" % (case, tag)]) < 1e-12        # same numpy pinv / solve: exact here
        Vgh, grads, _ = mos.variance_GH(m, nohess=True)
        assert rel_err(Vgh, G["%s_Vgh_%s" % (case, tag)]) < 1e-12
        for o in range(n_out):       # measured <= 1.7e-6 (output 0, cond(Phi) 1.8e10: the reference's gradK_c is -ffast-math)
            assert rel_err(grads[o][::7], G["%s_grad%d_%s_sub" % (case, o, tag)]) < 1e-5
            assert abs(np.linalg.norm(grads[o]) / float(G["%s_grad%d_%s_norm" % (case, o, tag)]) - 1) < 1e-5


@pytest.mark.parametrize("fname", ["spg_traj_n6.npz", "spg_traj_n12_k4.npz"])
def test_spg_trajectory(oracle, fname):
    """oracle spg()+callbacks reproduce the reference spg() run call by call (every f evaluated, every |g|)"""
    G = golden(fname)
    n, kmax = int(G["n"]), int(G["kmax"])
    prob = synth.problem(n, kmax, 1)
    sap = oracle.OracleSAP(prob["C"][0], kmax, prob["groups"], prob["costs"])
    scale = prob["budget"] / prob["costs"]
    fvals, gnorms = [], []

    def feval(x):
        try:
            f = sap.variance(scale * x)
        except AssertionError:
            f = np.inf
        fvals.append(f)
        return f

    def geval(x):
        g = scale * sap.variance_GH(scale * x, nohess=True)[1]
        gnorms.append(np.linalg.norm(g))
        return g

    res = oracle.spg(feval, geval, oracle.simplex_projection, np.ones(sap.L) / sap.L, eps=float(G["eps"]),
                     maxit=int(G["maxit"]), max_fevals=10 ** 5)
    assert res["it"] == int(G["it"]) and res["count"] == int(G["count"]) and res["solver_info"] == int(G["solver_info"])
    assert len(fvals) == len(G["fvals"])
    fin = np.isfinite(G["fvals"])
    assert (np.isfinite(fvals) == fin).all()
    assert rel_err(np.array(fvals)[fin], G["fvals"][fin]) < 1e-9
    assert rel_err(gnorms, G["gnorms"]) < 1e-7
    assert abs(res["f"] / float(G["f"]) - 1) < 1e-9
    assert rel_err(res["x"], G["x"]) < 1e-6


def test_simplex_projection_properties(oracle):
    rng = np.random.RandomState(3)
    for scale in (1.0, 1e-8, 1e30):
        v = scale * rng.randn(1000)
        x = oracle.simplex_projection(v)
        assert x.min() >= 0 and abs(x.sum() - 1) < 1e-12
        # idempotent, shift-invariant
        assert np.allclose(oracle.simplex_projection(x), x, atol=1e-15)
        if scale <= 1:
            assert np.allclose(oracle.simplex_projection(v + 7.0 * scale), x, atol=1e-12)
    # optimality: x = max(v - tau, 0) for one tau
    v = rng.randn(50)
    x = oracle.simplex_projection(v)
    tau = (v - x)[x > 0]
    assert np.ptp(tau) < 1e-12 and (v[x == 0] <= tau[0] + 1e-12).all()


def test_weighted_simplex_projection(oracle):
    rng = np.random.RandomState(4)
    u = rng.randn(500)
    assert np.allclose(oracle.weighted_simplex_projection(u, np.ones(500)), oracle.simplex_projection(u), atol=1e-15)
    s = rng.rand(500) + 1e-6
    p = oracle.weighted_simplex_projection(u, s)
    assert p.min() >= 0 and abs(p.sum() - 1) < 1e-12
    # KKT of the weighted problem: (p-u)/s = -tau on the support, >= -tau off it
    t = ((u - p) / s)
    assert np.ptp(t[p > 0]) < 1e-10 and (t[p == 0] <= t[p > 0].max() + 1e-10).all()


def test_reference_native_module_agrees_with_restatement(oracle):
    """the reference's own compiled cmisc.cpp vs the C restatement, and the 'as executed' evaluation used as bench.py's
    reference-kind CPU baseline: always against the module's recorded outputs (tests/golden/ref_native_n10_k4.npz,
    oracle/gen_golden.py), and against the live module where oracle/_ref is built.  The live check runs in a subprocess:
    oracle/_ref carries the reference's -ffast-math, and importing it would switch the whole pytest process to flush-to-zero."""
    import glob
    import os
    import subprocess
    import sys
    G = golden("ref_native_n10_k4.npz")
    n, kmax = int(G["n"]), int(G["kmax"])
    prob = synth.problem(n, kmax, 1)
    sap = oracle.OracleSAP(prob["C"][0], kmax, prob["groups"], prob["costs"])
    m = prob["m"][0]
    Vb, gb, _ = sap.variance_GH(m, nohess=True)
    assert abs(G["V_as_executed"] / Vb - 1) < 1e-14 and np.abs(G["grad_as_executed"] - gb).max() / np.abs(gb).max() < 1e-14
    for k in (1, 3):
        ours = oracle.objectiveK(n, k, sap.sizes[k], m[sap.cumsizes[k - 1]:sap.cumsizes[k]], sap.groups[k - 1], sap.invcovs[k - 1])
        assert np.abs(G["PHI_k%d" % k] - ours).max() / np.abs(ours).max() < 1e-15
    root = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
    if not glob.glob(os.path.join(root, "oracle", "_ref", "_cmisc_bluest*.so")):
        return                                  # oracle/_ref is built only where the reference tree is present
    code = """
import numpy as np
from oracle import oracle
from bluest_amd import synth
cm = oracle.ref_native()
prob = synth.problem(10, 4, 1)
sap = oracle.OracleSAP(prob["C"][0], 4, prob["groups"], prob["costs"])
m = prob["m"][0]
Va, ga, _ = sap.variance_GH_as_executed(m)
Vb, gb, _ = sap.variance_GH(m, nohess=True)
assert abs(Va / Vb - 1) < 1e-14 and np.abs(ga - gb).max() / np.abs(gb).max() < 1e-14
for k in (1, 3):
    PHI = np.zeros(100)
    args = (10, k, sap.sizes[k], m[sap.cumsizes[k - 1]:sap.cumsizes[k]])
    cm.objectiveK_c(PHI, *args, sap.groups[k - 1].ravel(), sap.invcovs[k - 1])
    ours = oracle.objectiveK(*args, sap.groups[k - 1], sap.invcovs[k - 1])
    assert np.abs(PHI - ours).max() / np.abs(ours).max() < 1e-15
print("ok")
"""
    out = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, cwd=root, timeout=300)
    assert out.returncode == 0 and "ok" in out.stdout, out.stdout + out.stderr


def test_checker_does_not_change_the_floating_point_environment(oracle):
    """the oracle the tests load is the strict-IEEE build: subnormals survive in this process after using it"""
    oracle.lib()
    tiny = np.float64(5e-324)
    assert tiny > 0 and np.float64(1e-310) * np.float64(0.5) > 0
    assert np.finfo(np.float64).smallest_subnormal > 0


def _estimator_case(G, case, sizes):
    samples, flat = G["samples%d" % case], G["sums%d" % case]
    sums, off = [], 0
    for k in range(1, len(sizes)):
        for i in range(sizes[k]):
            sums.append(list(flat[off:off + k]))
            off += k
    return samples, sums


def test_blue_estimator_vs_reference_fixture():
    """compute_BLUE_estimator (sap.py:99-119 + misc.py:518-544) restated in the oracle vs values recorded from the reference,
    including a case where some models are never sampled (restricted system)"""
    from oracle import oracle
    G = golden("estimator_n6_known_answers.npz")
    n, kmax = int(G["n"]), int(G["kmax"])
    prob = synth.problem(n, kmax, 1)
    sap = oracle.OracleSAP(prob["C"][0], kmax, [g.copy() for g in prob["groups"]], prob["costs"])
    for case in range(3):
        samples, sums = _estimator_case(G, case, sap.sizes)
        mu, var = sap.compute_BLUE_estimator(sums, samples)
        assert abs(mu / float(G["mu%d" % case]) - 1) < 1e-12 and abs(var / float(G["var%d" % case]) - 1) < 1e-12


def test_sparse_oracle_and_optimality_certificate(oracle):
    """SparseOracleSAP (Phi by the objectiveK_c loop) equals OracleSAP (dense psi@m, as the reference executes); the duality
    certificate is ~0 at an optimum found by an independent method (multiplicative algorithm on the CPU) and large elsewhere"""
    prob = synth.problem(7, 3, 2)
    m = prob["m"][0]
    for o in range(2):
        full = oracle.OracleSAP(prob["C"][o], 3, prob["groups"], prob["costs"])
        sp = oracle.SparseOracleSAP(prob["C"][o], 3, prob["groups"])
        Vf, gf, _ = full.variance_GH(m, nohess=True)
        Vs, gs, _ = sp.variance_GH(m)
        assert abs(Vs / Vf - 1) < 1e-13 and rel_err(gs, gf) < 1e-13 and abs(sp.variance(m) / full.variance(m) - 1) < 1e-13
        msp = m.copy(); msp[full.ES[6] == 1] = 0.0                 # model 6 unsampled: restricted solve, pinv gradient
        assert abs(sp.variance_GH(msp)[0] / full.variance_GH(msp, nohess=True)[0] - 1) < 1e-12
    # single output: multiplicative algorithm x_i <- x_i * (-dV/dx_i) / sum (monotone for c-optimal design)
    sp = oracle.SparseOracleSAP(prob["C"][0], 3, prob["groups"])
    w, B = prob["costs"], prob["budget"]
    scale = B / w
    x = np.ones(sp.L) / sp.L
    for it in range(4000):
        V, g, _ = sp.variance_GH(scale * x)
        x = x * (-(scale * g))
        x /= x.sum()
    V = sp.variance(scale * x)
    gap, lb, mu, info = oracle.optimality_certificate([sp], scale * x, w)
    assert -1e-10 <= gap < 1e-6 and lb <= V * (1 + 1e-10), (gap, info)
    touched = np.unique(np.concatenate([g[x[c0:c1] > 1e-8].ravel() for g, c0, c1 in zip(sp.groups, sp.cumsizes, sp.cumsizes[1:])]))
    assert len(touched) < sp.N                           # this optimum leaves models unsampled: the solved dual still closes the gap
    gap_u = oracle.optimality_certificate([sp], scale / sp.L, w)[0]
    assert gap_u > 0.05
    # two outputs: the bound is valid (<= F at ANY feasible point, here random ones and sparse ones)
    sps = [oracle.SparseOracleSAP(prob["C"][o], 3, prob["groups"]) for o in range(2)]
    rng = np.random.RandomState(0)
    pts = [rng.dirichlet(np.ones(sp.L)) for _ in range(3)]
    sparse = np.zeros(sp.L); sparse[[0, 9, 30]] = [0.5, 0.3, 0.2]
    pts.append(sparse)
    Fs, lbs = [], []
    for p in pts:
        gap, lb, mu, info = oracle.optimality_certificate(sps, scale * p, w)
        Fs.append(max(q.variance(scale * p) for q in sps))
        lbs.append(lb)
        assert gap >= -1e-10
    assert max(lbs) <= min(Fs) * (1 + 1e-10)                      # every lower bound is below every attained value


def test_singular_phi_fixture(oracle):
    """rank-deficient Phi with every model touched (two perfectly correlated models): the oracle reproduces what the reference's
    pinv-based variance_GH returns (misc.py:487,490); the reference's solve-based variance (misc.py:472) returns a different
    number for the same point -- the fixture records both"""
    G = golden("singular_phi_known_answer.npz")
    groups = [G["g_k%d" % k] for k in (1, 2, 3)]
    sap = oracle.OracleSAP(G["C"], 3, groups, np.ones(8))
    assert rel_err(np.concatenate(sap.invcovs), G["invcovs"]) < 1e-12
    assert rel_err(sap.get_phi(G["m"]), G["PHI"]) < 1e-13
    V, g, _ = sap.variance_GH(G["m"], nohess=True)
    assert abs(V / float(G["Vgh_pinv"]) - 1) < 1e-9 and rel_err(g, G["grad_pinv"]) < 1e-9
    assert abs(float(G["eigmin"])) < 1e-14 and int(G["variance_asserted"]) == 0
    assert abs(float(G["variance_solve"]) / float(G["Vgh_pinv"]) - 1) > 0.5          # the reference disagrees with itself here


def _support_problem_cpu(oracle, prob, keep, eps_bg, s):
    from oracle.master_newton import SupportProblem
    n, kmax, n_out = prob["n"], prob["kmax"], prob["n_out"]
    saps = [oracle.SparseOracleSAP(C, kmax, prob["groups"]) for C in prob["C"]]
    sp0 = saps[0]
    flat = [g for gk in sp0.groups for g in gk]
    c = prob["budget"] / prob["costs"]

    def block(o, i):
        k = int(np.searchsorted(sp0.cumsizes, i, side="right"))
        return saps[o].invcovs[k - 1].reshape(-1, k, k)[i - sp0.cumsizes[k - 1]]
    phi_u = np.array([q.get_phi(c / sp0.L) for q in saps])
    return SupportProblem(n, [flat[i] for i in keep], [[block(o, i) for i in keep] for o in range(n_out)], c[keep], s, eps_bg * phi_u, eps_bg), flat, c


@pytest.mark.parametrize("n,kmax,n_out,S", [(8, 3, 1, 20), (10, 4, 2, 30)])
def test_master_newton_restatement_against_slsqp(oracle, n, kmax, n_out, S):
    """oracle/master_newton.py (the numpy restatement of the GPU master, csrc/newton.hip): on a random support it reaches the
    optimum scipy's SLSQP finds for the same smooth problem, without and with per-model sample caps (max_model_samples)"""
    from scipy.optimize import minimize
    from oracle.master_newton import master_newton
    prob = synth.problem(n, kmax, n_out)
    rng = np.random.RandomState(5)
    keep = np.sort(np.concatenate([[0], 1 + rng.choice(prob["K_tot"] - 1, S - 1, replace=False)]))
    eps_bg = 1e-3
    sp, flat, cc = _support_problem_cpu(oracle, prob, keep, eps_bg, np.ones(n_out))
    x0 = np.full(S, 1.0 / S)
    ref = master_newton(sp, x0, tol=1e-10)
    assert ref["kkt"] <= 1e-6 and abs(ref["x"].sum() - 1) < 1e-12 and ref["x"].min() >= 0
    fun = lambda z: sp.evaluate(np.maximum(z, 0) / np.maximum(z, 0).sum()).max() * 1e3       # noqa: E731
    sol = minimize(fun, 0.9 * ref["x"] + 0.1 * x0, method="SLSQP", bounds=[(0, 1)] * S, constraints=[{"type": "eq", "fun": lambda z: z.sum() - 1}],
                   options={"ftol": 1e-15, "maxiter": 500})
    assert ref["F"] <= sol.fun / 1e3 * (1 + 1e-7)
    # caps on models 0 and 1 at 60 % of what the unconstrained optimum samples
    A = np.array([[cc[i] * (1 - eps_bg) if mdl in flat[i] else 0.0 for i in keep] for mdl in (0, 1)])
    b = 0.6 * (A @ ref["x"])
    x = x0.copy()
    for _ in range(200):                                    # a feasible start: shrink the capped groups
        viol = A @ x - b
        if (viol <= 0).all():
            break
        c_ = int(np.argmax(viol / b))
        msk = A[c_] > 0
        x[msk] *= 0.95 * b[c_] / (A[c_] @ x)
        x[~msk] += (1 - x.sum()) * x[~msk] / x[~msk].sum()
    capped = master_newton(sp, x, tol=1e-10, caps=(A, b))
    assert (A @ capped["x"] <= b * (1 + 1e-9)).all() and capped["nu"].min() >= 0 and capped["F"] > ref["F"]
    cons = [{"type": "eq", "fun": lambda z: z.sum() - 1}, {"type": "ineq", "fun": lambda z: b - A @ z}]
    sol = minimize(fun, 0.9 * capped["x"] + 0.1 * x, method="SLSQP", bounds=[(0, 1)] * S, constraints=cons, options={"ftol": 1e-15, "maxiter": 500})
    assert capped["F"] <= sol.fun / 1e3 * (1 + 1e-6), (capped["F"], sol.fun / 1e3)

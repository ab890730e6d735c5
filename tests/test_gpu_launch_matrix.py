"""
The evaluation m -> (Phi, V, grad V, status) in every kernel instantiation the plan can pick, against an 80-bit restatement
(oracle/ld_eval.py).  Each case of CASES is a plan shape with the launch configuration it must get -- asserted through
Plan.launch_config, i.e. through the helpers the launchers call --; test_cases_cover_every_instantiation (CPU) checks that the
expectations of the table cover every value of every instantiation set the library reports (bluest_amd.plan.launch_sets), so a new
instantiation that no case reaches, or a case taken out of the table, fails there.

Tolerances (u = eps/2 of float64, written next to each assert):
  Phi      every entry is a float64 sum of n_ab products: |err_ab| <= n_ab eps sum_i |t_i,ab| (no cancellation assumed)
  V, grad  a perturbation of relative size d of Phi moves V and y by cond(Phi) d, the elimination adds cond(Phi) N eps:
           cond (phi_rel + N eps); grad_i = -y_g^T B y_g doubles it.  Capped at the bars of the parity tests (1e-12 Phi, 1e-11
           V / grad on stored inverses, 1e-10 matrix-free as in test_gpu_matfree.py) on well-conditioned Phi; the ill-conditioned
           candidate of every case (cond ~ 1e7..1e9) is held to the derived bound itself.
"""
import ctypes

import numpy as np
import pytest

from bluest_amd import synth
from conftest import rel_err
from oracle import ld_eval

EPS = ld_eval.EPS
DELTAS = (0.0, 1e-3)
ENV_KEYS = ("BLUEST_MATFREE", "BLUEST_COLS32", "BLUEST_TILE_NT", "BLUEST_NO_REGULAR_FOLD")
NC = 6       # candidates of the batch: OK, INF, NO_MODEL0, SINGULAR, sparse OK, ill-conditioned OK
OK, INF, NOM0, SING, SPARSE, ILL = range(NC)


def case(name, n, profile, n_out, expect, ragged=False, env=None, path1=1):
    return dict(name=name, n=n, profile=profile, n_out=n_out, ragged=ragged, env=env or {}, expect=expect, path1=path1)


def _stored(nt, ku_sg, ku_gt, ob, tpb, cols16=1):
    return dict(phi_ob=ob, cols16=cols16, nt=nt, fold_threads=1024 if nt <= 26 else 256, solve_grad_ku=ku_sg, fused_tpb=tpb,
                grad_tiles_ku=ku_gt, matfree=0)


def _mf(nt, ku, nw, ob=0, mode=1):
    return dict(matfree=mode, mf_nt=nt, mf_ku=ku, mf_nw=nw, phi_ob=ob)


# profile: k -> "all" (every k-subset) or a count of random distinct k-subsets; the N singletons are always there (Phi regular)
CASES = [
    case("n8_k5_o3", 8, {2: "all", 3: "all", 4: "all", 5: "all"}, 3, _stored(8, 5, 5, 2, 15)),                  # OB 2, tail
    case("n12_k6_o2", 12, {2: "all", 3: 120, 5: 120, 6: 120}, 2, _stored(12, 6, 8, 2, 15)),                    # OB 2, no tail
    case("n16_k8_o1", 16, {2: "all", 3: 150, 7: 80, 8: 80}, 1, _stored(16, 8, 8, 0, 15)),                      # plain Phi kernel
    case("n20_k12_ragged_o3", 20, {2: "all", 4: 150, 9: 70, 11: 70, 12: 70}, 3, _stored(20, 12, 12, 0, 7), ragged=True),
    case("n26_k17_o2_cols32", 26, {2: "all", 5: 100, 13: 64, 17: 64}, 2, _stored(26, 12, 12, 2, 7, cols16=0),
         env={"BLUEST_COLS32": "1"}),
    case("n32_k32_o1", 32, {2: "all", 20: 40, 32: 1}, 1, _stored(32, 12, 12, 0, 7)),
    case("n40_k4_o2_ragged", 40, {2: "all", 3: 200, 4: 200}, 2, _stored(48, 5, 5, 0, 7), ragged=True),
    case("n64_k2_o16", 64, {2: "all"}, 16, _stored(64, 5, 5, 8, 7)),                                            # OB 8, no tail
    case("n64_k2_o12", 64, {2: "all"}, 12, _stored(64, 5, 5, 8, 7)),                                            # OB 8, tail of 4
    case("n64_k2_o8", 64, {2: "all"}, 8, _stored(64, 5, 5, 4, 7)),                                              # OB 4, no tail
    case("n64_k2_o5", 64, {2: "all"}, 5, _stored(64, 5, 5, 4, 7)),                                              # OB 4, tail of 1
    case("n64_k14_o2_ragged", 64, {2: 300, 6: 100, 14: 64}, 2, _stored(64, 12, 12, 0, 7), ragged=True),
    # matrix-free (BLUEST_MATFREE=1: Phi and gradient; =2: the gradient behind the stored Phi pass)
    case("mf_n8_k5", 8, {2: "all", 3: "all", 5: "all"}, 1, _mf(8, 5, 8), env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mf_n12_k6_o2", 12, {2: "all", 4: 100, 6: 100}, 2, _mf(12, 6, 8, ob=2), env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mf_n16_k8", 16, {2: "all", 7: 60, 8: 60}, 1, _mf(16, 8, 8), env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mf_n20_k4", 20, {2: "all", 4: 150}, 1, _mf(20, 5, 8), env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mf_n26_k3_o2_ragged", 26, {2: "all", 3: 200}, 2, _mf(26, 5, 8), ragged=True, env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mf_n32_k6", 32, {2: "all", 6: 100}, 1, _mf(32, 6, 8), env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mf_n48_k8", 48, {2: "all", 8: 100}, 1, _mf(48, 8, 4), env={"BLUEST_MATFREE": "1"}, path1=2),
    case("mfgrad_n40_k8_o2", 40, {2: "all", 5: 100, 8: 64}, 2, _mf(48, 8, 4, ob=2, mode=2), env={"BLUEST_MATFREE": "2"}, path1=3),
]


def _groups(n, profile, rng):
    """list over k = 1..K of (L_k, k) int64 arrays, lexicographic inside each size"""
    K = max(profile)
    out = []
    for k in range(1, K + 1):
        if k == 1:
            g = np.arange(n).reshape(-1, 1)
        elif profile.get(k) == "all":
            g = synth.all_groups(n, k)[k - 1]
        elif k in profile:
            seen = set()
            while len(seen) < profile[k]:
                seen.add(tuple(sorted(rng.choice(n, k, replace=False).tolist())))
            g = np.array(sorted(seen), dtype=np.int64).reshape(-1, k)
        else:
            g = np.zeros((0, k), dtype=np.int64)
        out.append(np.asarray(g, dtype=np.int64))
    return out


def _problem(c):
    """plan description + host copies: global groups, per output (local groups, mapping)"""
    rng = np.random.RandomState(sum(map(ord, c["name"])))
    n, K = c["n"], max(c["profile"])
    G = _groups(n, c["profile"], rng)
    sizes = np.array([len(g) for g in G])
    L = int(sizes.sum())
    outs, host = [], []
    for o in range(c["n_out"]):
        C = synth.wishart_covariance(n, o)[0]
        if c["ragged"]:
            keep = [np.ones(len(g), bool) if k == 1 else rng.rand(len(g)) < 0.7 for k, g in enumerate(G, start=1)]
        else:
            keep = [np.ones(len(g), bool) for g in G]
        gl = [g[kk] for g, kk in zip(G, keep)]
        first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
        mapping = np.concatenate([f + np.flatnonzero(kk) for f, kk in zip(first, keep)]).astype(np.int64)
        outs.append({"K": K, "sizes": [len(g) for g in gl], "groups": gl, "C": C, "mapping": mapping if c["ragged"] else None})
        host.append((gl, mapping, C))
    return G, L, outs, host


def _candidates(G, L, n, rng):
    has = lambda model: np.concatenate([(g == model).any(axis=1) for g in G])      # noqa: E731
    M = np.empty((NC, L))
    M[OK] = 0.5 + rng.rand(L)
    M[INF] = 0.01                                                  # max|m| < 0.05 (misc.py:464)
    M[NOM0] = M[OK] * ~has(0)                                      # model 0 not sampled
    M[SING] = -M[OK]                                               # Phi negative definite: no positive pivot
    single = np.concatenate([np.full(len(g), k == 1) for k, g in enumerate(G, start=1)])
    M[SPARSE] = M[OK] * ((rng.rand(L) < 0.4) | single)
    M[ILL] = M[OK] * np.where(has(n - 1), 1e-5, 1.0)               # model n-1 seen 1e5 times weaker: cond(Phi) ~ 1e7..1e9
    return M


def _bounds(ref, N, phi_abs, cnt, matfree, kcond=0.0):
    """(phi_rel, V / grad bound) of one (candidate, output), see the module docstring"""
    scale = float(np.abs(ref["phi"]).max())
    phi_rel = float((cnt * EPS * phi_abs.astype(np.float64)).max()) / scale
    if matfree:                                    # the group factors are recomputed in float64: k cond(C_g) eps per term
        phi_rel += kcond * EPS * float(phi_abs.astype(np.float64).max()) / scale
    phi_tol = min(1e-12, phi_rel)
    derived = 2.0 * ref["cond"] * (phi_rel + N * EPS)
    cap = 1e-10 if matfree else 1e-11
    return phi_tol, (derived if ref["cond"] > 1e6 else min(cap, derived))


def _ref_blocks(plan, host, matfree):
    out = []
    for o, (gl, _, C) in enumerate(host):
        out.append(ld_eval.blocks_from_cov(C, gl) if matfree else ld_eval.blocks_from_flat([len(g) for g in gl], plan.invcovs[o]))
    return out


def _kcond(host):
    """largest k cond(C_g) over the groups of the plan (the error scale of a recomputed group factor)"""
    worst = 0.0
    for gl, _, C in host:
        for k, g in enumerate(gl, start=1):
            if len(g) and k > 1:
                sub = C[g[:, :, None], g[:, None, :]]
                worst = max(worst, k * float(np.linalg.cond(sub).max()))
    return worst


@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


def test_cases_cover_every_instantiation():
    """CPU: the expected configurations of CASES reach every value of every instantiation set the library is built with"""
    from bluest_amd.plan import launch_sets
    sets = launch_sets()
    seen = {axis: set() for axis in sets}
    ob_multiple, ob_tail = set(), set()
    plain = cols = False
    generic_nt = set()             # NT of the stored cases with groups wider than 12 (grad_tile_generic in both gradient families)
    paths = set()
    for c in CASES:
        e = c["expect"]
        stored = e["matfree"] == 0
        paths.add(c["path1"])
        for axis in sets:
            if axis.startswith("mf_") and e["matfree"] == 0:
                continue
            if axis == "mf_nw" and e["matfree"] != 1:
                continue                                   # k_phi_matfree<NW> only runs with the matrix-free Phi pass
            if axis in e and (stored or axis.startswith("mf_") or axis == "phi_ob"):
                seen[axis].add(e[axis])
        if e["phi_ob"]:
            (ob_multiple if c["n_out"] % e["phi_ob"] == 0 else ob_tail).add(e["phi_ob"])
        plain = plain or e["phi_ob"] == 0
        cols = cols or e.get("cols16") == 0
        if stored and max(c["profile"]) > 12:
            generic_nt.add(e["nt"])
    for axis, values in sets.items():
        missing = set(values) - seen[axis]
        assert not missing, "no case reaches %s = %s" % (axis, sorted(missing))
    assert ob_multiple >= set(sets["phi_ob"]) and ob_tail >= set(sets["phi_ob"]), (ob_multiple, ob_tail)
    assert plain and cols
    # single-candidate paths: fused k_solve_grad, matrix-free Phi + gradient, stored Phi + matrix-free gradient
    assert paths == {1, 2, 3}, paths
    # groups wider than 12 at NT <= 26 (1024-thread fold), NT > 26, and at the widest NT (model index bytes up to 63)
    assert min(generic_nt) <= 26 < max(generic_nt) and max(sets["nt"]) in generic_nt, generic_nt


@pytest.mark.gpu
@pytest.mark.parametrize("c", CASES, ids=[c["name"] for c in CASES])
def test_instantiation_against_ld_reference(gpu, monkeypatch, c):
    torch = gpu
    from bluest_amd import _lib
    from bluest_amd.plan import Plan
    for k_ in ENV_KEYS:
        monkeypatch.delenv(k_, raising=False)
    for k_, v_ in c["env"].items():
        monkeypatch.setenv(k_, v_)
    n, n_out = c["n"], c["n_out"]
    G, L, outs, host = _problem(c)
    plan = Plan(n, L, outs, max_candidates=NC)
    # ---- the launch configuration the case is about
    cfg1, cfgb = plan.launch_config(1), plan.launch_config(NC)
    for key, want in c["expect"].items():
        assert cfg1[key] == want, (c["name"], key, cfg1)
    assert cfg1["path"] == c["path1"] and cfgb["path"] == 0
    assert cfg1["kmax"] == max(c["profile"])
    matfree = cfg1["matfree"] != 0
    dev = plan.device
    rng = np.random.RandomState(7)
    M = _candidates(G, L, n, rng)
    Md = torch.from_numpy(M).to(dev)
    blocks = _ref_blocks(plan, host, matfree)
    kcond = _kcond(host) if matfree else 0.0
    refs = {}
    for ci in range(NC):
        for o, (gl, mapping, _) in enumerate(host):
            mloc = M[ci][mapping]
            for delta in DELTAS:
                r = ld_eval.evaluate(n, gl, blocks[o], mloc, delta=delta)
                if r["phi"] is not None:
                    pa, cnt = ld_eval.phi_ld(n, gl, blocks[o], mloc, absolute=True)
                    r["tol"] = _bounds(r, n, pa, cnt, matfree, kcond)
                refs[ci, o, delta] = r
    N2 = n * n

    def check_phi(rec, ci_list, label):
        rec = rec.cpu().numpy()
        for j, ci in enumerate(ci_list):
            for o in range(n_out):
                r = refs[ci, o, 0.0]
                t = rec[j, o]
                big = np.abs(M[ci][host[o][1]]).max() >= 0.05
                assert t[N2 + 2 * n] == (1.0 if big else 0.0), (label, ci, o)
                if r["phi"] is None:
                    continue
                # Phi: n_ab eps sum|t| (capped at 1e-12)
                assert rel_err(t[:N2].reshape(n, n), r["phi"].astype(np.float64)) <= r["tol"][0], (label, ci, o)
                m_loc = M[ci][host[o][1]]
                t1, t2 = np.zeros(n), np.zeros(n)
                for k, g in enumerate(host[o][0], start=1):
                    sel = np.concatenate([[0], np.cumsum([len(x) for x in host[o][0]])])
                    mk = m_loc[sel[k - 1]:sel[k]]
                    t1[g[np.abs(mk) > 1e-6].ravel()] = 1.0
                    t2[g[mk != 0].ravel()] = 1.0
                assert np.array_equal(t[N2:N2 + n], t1) and np.array_equal(t[N2 + n:N2 + 2 * n], t2), (label, ci, o)

    def check_eval(var, grad, st, ci_list, delta, label, want_grad=True):
        var, st = var.cpu().numpy(), st.cpu().numpy()
        grad = grad.cpu().numpy() if want_grad else None
        for j, ci in enumerate(ci_list):
            for o in range(n_out):
                r = refs[ci, o, delta]
                tag = (c["name"], label, ci, o, delta)
                if ci == SING:
                    # judged against the float64 semantics: the restricted Phi is not positive definite -> SINGULAR, V = NaN
                    assert np.linalg.eigvalsh(r["phi"][np.ix_(r["idx"], r["idx"])].astype(np.float64)).min() <= 0
                    assert st[j, o] == 3 and np.isnan(var[j, o]), tag
                    continue
                assert st[j, o] == r["status"], tag
                g = grad[j, plan.grad_off[o]:plan.grad_off[o] + len(host[o][1])] if want_grad else None
                if r["status"] == ld_eval.EVAL_INF:
                    assert np.isinf(var[j, o]) and (not want_grad or np.isinf(g).all()), tag
                    continue
                tol = r["tol"][1]
                assert abs(var[j, o] / r["V"] - 1) <= tol, tag + (var[j, o], r["V"], tol, r["cond"])
                if want_grad:
                    if not r["grad"].any():
                        assert not g.any(), tag
                    else:
                        assert rel_err(g, r["grad"]) <= 2 * tol, tag + (rel_err(g, r["grad"]), tol)

    everyone = list(range(NC))
    # ---- Phi records: batch, then one by one (matrix-free plans: k_phi_matfree at n_cand = 1)
    rec_b = plan.phi(Md)
    check_phi(rec_b, everyone, "phi batch")
    for ci in (OK, ILL):
        check_phi(plan.phi(Md[ci]), [ci], "phi single")
    for delta in DELTAS:
        var_b, grad_b, st_b = plan.eval(Md, delta=delta)
        check_eval(var_b, grad_b, st_b, everyone, delta, "eval batch")
        vw, _, sw = plan.eval(Md, delta=delta, want_grad=False)
        assert torch.equal(st_b, sw) and torch.equal(var_b.nan_to_num(7.0), vw.nan_to_num(7.0))
        # one by one: the single-candidate kernels (fused k_solve_grad / matrix-free) against the batch kernels
        for ci in everyone:
            v1, g1, s1 = plan.eval(Md[ci], delta=delta)
            check_eval(v1, g1, s1, [ci], delta, "eval single")
            assert torch.equal(s1[0], st_b[ci])
            if c["path1"] == 1:
                # same fold, elimination and tile arithmetic (tile_form<k> / grad_tile_generic in both): bit for bit
                assert torch.equal(v1[0].nan_to_num(7.0), var_b[ci].nan_to_num(7.0)), (c["name"], ci)
                assert torch.equal(g1[0].nan_to_num(7.0), grad_b[ci].nan_to_num(7.0)), (c["name"], ci)
        # split path phi -> solve -> grad (batch): the fold of k_fold_to_record, the elimination and k_grad_tiles of eval
        var3, v3, st3 = plan.solve(rec_b, delta=delta)
        grad3 = plan.grad(v3, st3)
        assert torch.equal(st3, st_b)
        assert torch.equal(var3.nan_to_num(7.0), var_b.nan_to_num(7.0)) and torch.equal(grad3.nan_to_num(7.0), grad_b.nan_to_num(7.0))
        # ... and for one candidate (matrix-free plans: k_phi_matfree record, elimination from the record, k_grad_mf)
        rec1 = plan.phi(Md[OK])
        var4, v4, st4 = plan.solve(rec1, delta=delta)
        grad4 = plan.grad(v4, st4)
        check_eval(var4, grad4, st4, [OK], delta, "split single")
        if c["path1"] == 1:
            assert torch.equal(var4[0], var_b[OK]) and torch.equal(grad4[0], grad_b[OK])
    # ---- raw C-ABI: m_stride > L, grad_stride > grad_len, poisoned padding that must stay untouched
    pad_m, pad_g = 5, 3
    Mp = torch.full((NC, L + pad_m), float("nan"), dtype=torch.float64, device=dev)
    Mp[:, :L] = Md
    var = torch.empty((NC, n_out), dtype=torch.float64, device=dev)
    st = torch.empty((NC, n_out), dtype=torch.int32, device=dev)
    gp = torch.full((NC, plan.grad_len + pad_g), 7.25, dtype=torch.float64, device=dev)
    with torch.cuda.device(dev):
        _lib.check(plan.lib.bluest_plan_eval(plan._h, Mp.data_ptr(), NC, L + pad_m, 1e-3, var.data_ptr(), gp.data_ptr(),
                                             plan.grad_len + pad_g, st.data_ptr(), ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)))
    torch.cuda.synchronize()
    assert bool((gp[:, plan.grad_len:] == 7.25).all()) and bool(Mp[:, L:].isnan().all())
    assert torch.equal(st, st_b) and torch.equal(var.nan_to_num(7.0), var_b.nan_to_num(7.0))
    assert torch.equal(gp[:, :plan.grad_len].nan_to_num(7.0), grad_b.nan_to_num(7.0))
    # ---- combine_grad with n_cand > 1, with and without scale, against a longdouble sum
    fin = [OK, SPARSE, ILL]
    gsel = grad_b[fin].contiguous()
    coef = torch.from_numpy(rng.rand(len(fin), n_out)).to(dev)
    scale = torch.from_numpy(0.5 + rng.rand(L)).to(dev)
    gh, ch, sh = gsel.cpu().numpy().astype(np.longdouble), coef.cpu().numpy(), scale.cpu().numpy()
    for sc in (None, scale):
        got = plan.combine_grad(gsel, coef, scale=sc).cpu().numpy()
        want = np.zeros((len(fin), L), dtype=np.longdouble)
        mag = np.zeros((len(fin), L), dtype=np.longdouble)
        for o in range(n_out):
            mp = host[o][1]
            term = ch[:, o:o + 1] * gh[:, plan.grad_off[o]:plan.grad_off[o] + len(mp)]
            want[:, mp] += term
            mag[:, mp] += np.abs(term)
        if sc is not None:
            want, mag = want * sh, mag * sh
        # n_out fma steps and one product: (n_out + 1) eps sum |terms|, relative to the largest entry
        bound = (n_out + 1) * EPS * float(mag.max()) / float(np.abs(want).max())
        assert rel_err(got, want.astype(np.float64)) <= bound, (c["name"], sc is None)

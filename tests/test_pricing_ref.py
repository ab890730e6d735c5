"""
CPU checks of the pricing reference (oracle/pricing_ref.py) and of the case table (pricing_cases.py) that test_gpu_pricing.py
runs on the GPU: the reference agrees with the independent dual bound of oracle/master_newton.py on real gradients, and the
table reaches every path of k_price it claims to reach -- read off the reference's own results, not assumed.
"""
import numpy as np
import pytest

import pricing_cases as pc
from oracle import pricing_ref as ref
from oracle.master_newton import dual_bound

EPS = ref.DBL_EPS
CASES = pc.all_price_cases()
_refs = {}


def reference(c):
    if c["name"] not in _refs:
        a = pc.inputs(c)
        _refs[c["name"]] = (a, pc.reference(c, a))
    return _refs[c["name"]]


def test_fma_rounds_once():
    """(1 + e)(1 - e) + (-1) = -e^2 exactly; the separate product rounds to 1 and gives 0"""
    e = 2.0 ** -30
    assert (1.0 + e) * (1.0 - e) - 1.0 == 0.0 and ref.fma(1.0 + e, 1.0 - e, -1.0) == -e * e
    assert 0.1 * 10.0 - 1.0 == 0.0 and ref.fma(0.1, 10.0, -1.0) == 2.0 ** -54      # ten times the double next to 0.1 is 1 + 2^-54
    assert ref.fma(float("inf"), 2.0, 1.0) == float("inf") and np.isnan(ref.fma(float("inf"), 0.0, 1.0))


def _real_forms(sh, m):
    """q[o][i] = y_g^T C_g^-1 y_g with y = Phi_o(m)^-1 e_0 (q = -dV_o/dm_i), and y0[o] = y_0, in plain numpy"""
    G = np.concatenate([np.pad(g, ((0, 0), (0, sh["K"] - g.shape[1])), constant_values=-1) for g in pc.synth.all_groups(sh["n"], sh["K"])])
    q, v = np.zeros((sh["n_out"], sh["L"])), np.zeros((sh["n_out"], sh["n"]))
    for o, out in enumerate(sh["outs"]):
        inv = {}
        phi = np.zeros((sh["n"], sh["n"]))
        for i in sh["mappings"][o]:
            g = G[i][G[i] >= 0]
            inv[i] = np.linalg.inv(out["C"][np.ix_(g, g)])
            phi[np.ix_(g, g)] += m[i] * inv[i]
        y = np.linalg.solve(phi, np.eye(sh["n"])[0])
        v[o] = y
        for i in sh["mappings"][o]:
            g = G[i][G[i] >= 0]
            q[o, i] = y[g] @ inv[i] @ y[g]
    return q, v


@pytest.mark.parametrize("key,n_out,ragged", [("n6", 1, False), ("n6", 3, False), ("n6", 3, True), ("n12", 3, True)])
def test_reference_agrees_with_the_dual_bound_on_real_gradients(key, n_out, ragged):
    """c_i within (n_out + 2) eps sum|terms| of dual_bound's matrix product (n_out products and sums, the division mu/s, the
    product with cc), and the bound A^2 / (4 cmax) within the relative errors of its parts: twice A's, cmax's, 4 eps"""
    sh = pc.shape(key, n_out, ragged)
    rng = np.random.RandomState(3)
    b = pc.base_inputs(sh)
    q, v = _real_forms(sh, 0.5 + rng.rand(sh["L"]))
    grad = np.full(sh["grad_len_host"], pc.POISON)
    for o, mp in enumerate(sh["mappings"]):
        grad[sh["goff_host"][o]:sh["goff_host"][o] + len(mp)] = -q[o, mp]
    sup = pc.support(sh)
    res = ref.price(sh["L"], n_out, grad, sh["goff_host"], sh["invmap"], b["mu"], b["s"], b["cc"], len(sup), sup, v.ravel(), sh["n"])
    lb_ind, ci = dual_bound(q, v[:, 0], b["mu"], b["s"], b["cc"])
    a = b["mu"] / b["s"]
    tol_c = (n_out + 2) * EPS * b["cc"] * (a @ np.abs(q))
    assert (np.abs(res["c"] - ci) <= tol_c).all()
    assert np.array_equal(res["c_sup"], res["c"][sup]) and np.array_equal(res["y0"], v[:, 0])
    cmax, A, lb = ref.bound(res, b["mu"], b["s"], len(sup))
    assert cmax == res["c"].max()                      # the reported candidates hold the true maximum
    i = int(np.argmax(ci))
    rel = 2.0 * (n_out + 2) * EPS * float(a @ np.abs(v[:, 0])) / abs(A) + tol_c[i] / ci[i] + 4.0 * EPS
    assert abs(lb - lb_ind) <= rel * lb_ind, (lb, lb_ind, rel)


@pytest.mark.parametrize("name", [c["name"] for c in CASES if c["sh"]["L"] < 1000])
def test_case_references_equal_the_plain_restatement(name):
    """the column-wise shortcut of pricing_cases.reference gives what ref.price gives on the whole input"""
    c = next(c for c in CASES if c["name"] == name)
    a, r = reference(c)
    sh = c["sh"]
    full = ref.price(sh["L"], sh["n_out"], a["grad"], a["goff"], sh["invmap"], a["mu"], a["s"], a["cc"], len(a["sup"]), a["sup"], a["v_ws"],
                     sh["n"], a["capmask"], a["nu"], a["master_out"])
    for k in ("c", "c_sup", "top_val", "top_idx", "y0"):
        assert np.array_equal(full[k].view(np.int64), r[k].view(np.int64)), k


@pytest.mark.parametrize("name", [c["name"] for c in CASES])
def test_top_candidates_gives_the_head_of_the_full_sort(name):
    from bluest_amd.colgen import top_candidates
    _, r = reference(next(c for c in CASES if c["name"] == name))
    order = np.lexsort((r["top_idx"], -r["top_val"]))
    for k in (1, 5, 21, 64, 1023, 1024, 2000):
        ci, cv = top_candidates(r["top_val"], r["top_idx"], k)
        kk = min(k, 1024)
        assert ci[:kk] == r["top_idx"][order][:kk].tolist() and cv[:kk] == r["top_val"][order][:kk].tolist()


def _blocks(r):
    return r["top_val"].reshape(ref.PRICE_BLOCKS, ref.PRICE_TOP), r["top_idx"].reshape(ref.PRICE_BLOCKS, ref.PRICE_TOP)


def test_the_table_reaches_every_path():
    seen = set()
    for c in CASES:
        a, r = reference(c)
        sh, L = c["sh"], c["sh"]["L"]
        tv, ti = _blocks(r)
        cvec = r["c"]
        assert np.isfinite(cvec).all()
        # every workgroup's first entry is the maximum of what it scanned, at the smallest index attaining it
        for b in range(ref.PRICE_BLOCKS):
            mine = np.concatenate([np.arange(b * 256 + k * pc.STRIDE, min(b * 256 + k * pc.STRIDE + 256, L)) for k in range(2)]).astype(np.int64)
            if len(mine) == 0:
                assert (ti[b] == -1).all() and (tv[b] == -np.inf).all()
                seen.add("empty workgroup")
                continue
            assert tv[b, 0] == cvec[mine].max() and ti[b, 0] == mine[cvec[mine] == cvec[mine].max()].min()
            filled = int((ti[b] >= 0).sum())
            assert filled == min(ref.PRICE_TOP, len(set(mine % 256)))
            if filled < ref.PRICE_TOP:
                seen.add("partly filled workgroup")
            if (mine >= pc.STRIDE).any():
                seen.add("second round")
        if sh["ragged"]:
            seen.add("li < 0")
            sup = a["sup"]
            assert sup[0] == 0 and sup[-1] == L - 1 and (sh["invmap"][1][sup] < 0).any() and (np.diff(sup) > 0).all()
        if c["inf"]:
            assert a["mu"][1] == 0.0 and np.isinf(a["grad"]).any()
            seen.add("mu = 0 on an infinite gradient")
        if c["caps"]:
            assert a["capmask"].max() < 2 ** c["caps"] and len(a["nu"]) == 64
            if c["caps"] == 64:
                assert int(a["capmask"][L - 1]) >> 63 == 1
            if (cvec < 0).any():
                seen.add("negative capped reduced cost")
        for kind, i, j, f in c["expect"].get("ties", ()):
            assert i < j and cvec[i] == cvec[j] and np.array_equal(a["q"][:, i], a["q"][:, j]) and a["cc"][i] == a["cc"][j]
            bi, bj = pc.block_of(i), pc.block_of(j)
            if kind == "wave":
                assert bi == bj and pc.wave_of(i) == pc.wave_of(j) and pc.thread_of(i) != pc.thread_of(j)
            elif kind == "waves":
                assert bi == bj and pc.wave_of(i) != pc.wave_of(j)
            elif kind in ("workgroups", "rounds"):
                assert bi != bj
            if kind in ("wave", "waves"):                         # both reported, adjacent, the smaller index first
                k = int(np.flatnonzero(ti[bi] == i)[0])
                assert ti[bi, k + 1] == j and tv[bi, k] == tv[bi, k + 1]
            if kind == "stride":                                  # one thread met both and kept the first
                assert bi == bj and pc.thread_of(i) == pc.thread_of(j) and i in ti[bi] and j not in ti[bi]
            if kind == "rounds":                                  # the global maximum twice
                assert (i, j) == (pc.STRIDE - 1, pc.STRIDE) and cvec[i] == cvec.max() and int(np.flatnonzero(cvec == cvec.max())[0]) == i
            seen.add("tie: " + kind)
        if "argmax" in c["expect"]:
            i = c["expect"]["argmax"]
            assert int(np.argmax(cvec)) == i and (cvec == cvec[i]).sum() == 1 and ti[pc.block_of(i), 0] == i
            seen.add("maximum at %s" % {0: "0", L - 1: "L-1"}.get(i, str(i)))
        if "stride_pair" in c["expect"]:
            i, j = c["expect"]["stride_pair"]
            b = pc.block_of(i)
            mine = np.concatenate([np.arange(b * 256, b * 256 + 256), np.arange(b * 256 + pc.STRIDE, min(b * 256 + pc.STRIDE + 256, L))])
            top16 = mine[np.argsort(-cvec[mine], kind="stable")[:ref.PRICE_TOP]]
            assert pc.thread_of(i) == pc.thread_of(j) and i in top16 and j in top16 and j in ti[b] and i not in ti[b]
            seen.add("two of the top 16 on one stride")
    want = {"empty workgroup", "partly filled workgroup", "second round", "li < 0", "mu = 0 on an infinite gradient",
            "negative capped reduced cost", "tie: wave", "tie: waves", "tie: workgroups", "tie: stride", "tie: rounds",
            "maximum at 0", "maximum at L-1", "maximum at 16383", "maximum at 16384", "two of the top 16 on one stride"}
    assert want <= seen, want - seen


def test_support_point_roundings_differ_where_the_table_can_tell():
    """both roundings agree off the support and for eps = 0; on a 64-entry support with eps > 0 they differ somewhere, so the
    GPU test does identify the contraction the build took"""
    for name, L, S, sup, xs, cc, eps in pc.support_cases():
        sep, fused = ref.support_point(L, S, sup, xs, cc, eps)
        off = np.setdiff1d(np.arange(L), sup)
        assert np.array_equal(sep[off], fused[off]) and np.array_equal(sep[off], cc[off] * (eps / L))
        assert np.isclose((sep / cc).sum(), 1.0, rtol=1e-12, atol=0.0)
        if eps == 0.0:
            assert np.array_equal(sep, fused) and np.array_equal(sep[sup], cc[sup] * xs)
        elif S == 64:
            assert not np.array_equal(sep, fused), name


@pytest.mark.parametrize("key,n_out,ragged", pc.MA_SHAPES[:-1])
def test_ma_update_reference(key, n_out, ragged):
    """p = 1 and a single output weigh every output 1; the not-evaluable exits return the iterate untouched; on real gradients
    the step keeps sum x = 1 (V_o is homogeneous of degree -1) -- the restatement is the algorithm, not just the kernel's text"""
    sh = pc.shape(key, n_out, ragged)
    for fault in ("status", "inf", "zero"):
        a = pc.ma_inputs(sh, 32.0, fault=fault)
        x, m, facts = pc.ma_reference(sh, a)
        assert not facts["ok"] and np.array_equal(x, a["x"]) and np.array_equal(m, a["m"])
    a = pc.ma_inputs(sh, 1.0)
    assert pc.ma_reference(sh, a)[2]["w"] == [1.0] * n_out
    a = pc.ma_inputs(sh, 32.0)
    x, m, facts = pc.ma_reference(sh, a)
    assert facts["ok"] and max(facts["w"]) == 1.0 and (np.array(facts["w"]) > 0).all() and (x >= 0).all() and np.array_equal(m, a["cc"] * x)
    if n_out <= 3 and sh["L"] < 100:
        q, v = _real_forms(sh, a["m"])
        for o, mp in enumerate(sh["mappings"]):
            a["grad"][a["goff"][o]:a["goff"][o] + len(mp)] = -q[o, mp]
        a["var"] = v[:, 0].copy()
        x, m, facts = pc.ma_reference(sh, a)
        assert abs(x.sum() - 1.0) < 1e-12

"""
Plans, allocations and calls of tests/test_gpu_solve_grad_bits.py, shared with tools/gen_golden_solve_grad_bits.py (which recorded
tests/golden/solve_grad_bits_parent.npz).  numpy only; every input is seeded, so the fixture holds results only.

Each plan is the smallest that reaches one path of the fused solve + gradient kernel (k_solve_grad) and of the fold and solve it
shares with the other kernels.  All of them are small, so every workgroup owns ONE tile (tiles_per_wg = 1) of the 15 or 7 tile
wavefronts its instantiation has: wavefronts 2.. of every workgroup only fold.
  reg_n6_o2     n=6, all subsets to k=3, 2 outputs   equal workgroups per output (bpo = 3 > 0), pads (NT = 8), regular fold
  reg_n8_o3     n=8, all subsets to k=4, 3 outputs   bpo = 5 > 0 (two tiles of k = 4, the second with 6 groups), no pads (N = NT)
  ragged_o2     n=6, output 1 without the triples    3 and 2 workgroups: bpo == 0, output and `first` from the tile descriptor
  rowrag_o2     rows of unequal chunk counts         descriptor fold (FoldReg.Cd == 0), pads (n=11, NT = 12)
  pads_n10_o1   n=10, pairs                          pads (NT = 12), one output
  extra_n18_o2  n=18, pairs                          NT = 20: E = 4 extra rows of the DPP elimination, pads
  generic_n14   n=14, pairs + five groups of 13      tiles of k = 13 > 12: the generic tile path (KU = 12, 7 tile wavefronts)
  ma_n6_o1      n=6, all subsets to k=3, 1 output    identity plan: bluest_plan_eval_ma, the update in the tile wavefronts
Allocations (ALLOCS): all groups sampled; one model unsampled (identity row in place); model 0 unsampled (rows and columns
swapped, status NO_MODEL0); one model sampled below 1e-6 only (V's system and v's differ: the second pass of solve_wave).
Calls (CALLS): plan.eval with delta = 0 and delta != 0, and plan.solve_grad fed from plan.phi's record.
"""
import numpy as np

import step_bits_cases as sbc
from bluest_amd import synth

CUS = 256                     # compute units of the MI355X (layout_tiles spreads the tiles over them)
NT_SET = (8, 12, 16, 20, 26, 32, 48, 64)
KU_SET = (5, 6, 8, 12)
DELTA = 0.01


def _pairs_plus(n, extra):
    """singletons, every pair, and `extra` = {k: list of groups}; sizes without groups stay empty"""
    K = max([2] + list(extra))
    out = synth.all_groups(n, 2)
    for k in range(3, K + 1):
        out.append(np.array(sorted(extra.get(k, [])), dtype=np.int64).reshape(-1, k))
    return out


def _generic_groups():
    n = 14
    return _pairs_plus(n, {13: [tuple(i for i in range(n) if i != drop) for drop in (9, 10, 11, 12, 13)]})


#        name            n   groups                              n_out  output 1.. keep sizes <= this (None: all)  env
CASES = [
    ("reg_n6_o2", 6, lambda: synth.all_groups(6, 3), 2, None, {}),
    ("reg_n8_o3", 8, lambda: synth.all_groups(8, 4), 3, None, {}),
    ("ragged_o2", 6, lambda: synth.all_groups(6, 3), 2, 2, {}),
    ("rowrag_o2", 11, sbc._rowrag_groups, 2, None, {"BLUEST_NO_REGULAR_FOLD": "1"}),
    ("pads_n10_o1", 10, lambda: synth.all_groups(10, 2), 1, None, {}),
    ("extra_n18_o2", 18, lambda: synth.all_groups(18, 2), 2, None, {}),
    ("generic_n14", 14, _generic_groups, 1, None, {}),
    ("ma_n6_o1", 6, lambda: synth.all_groups(6, 3), 1, None, {}),
]
NAMES = [c[0] for c in CASES]
ALLOCS = ("ok", "no3", "no0", "tiny2")
#        label    allocation  delta  from the record?
CALLS = [("ok", "ok", 0.0, False), ("no3", "no3", 0.0, False), ("no0", "no0", 0.0, False), ("tiny2", "tiny2", 0.0, False),
         ("ok_d", "ok", DELTA, False), ("no3_d", "no3", DELTA, False), ("ok_rec", "ok", 0.0, True), ("tiny2_rec_d", "tiny2", DELTA, True)]
MA_STEPS = 3
ENV_KEYS = ("BLUEST_MATFREE", "BLUEST_COLS32", "BLUEST_TILE_NT", "BLUEST_NO_REGULAR_FOLD", "BLUEST_PHI_OB")


def pick(values, x):
    return next((v for v in values if x <= v), values[-1])


def problem(name):
    """dict: n, L (global groups), outs (for Plan()), groups (global), local (per output: groups, mapping), env, allocs {kind: m}"""
    i = NAMES.index(name)
    _, n, mk, n_out, keep_k, env = CASES[i]
    G = mk()
    sizes = np.array([len(g) for g in G])
    L = int(sizes.sum())
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    outs, local = [], []
    for o in range(n_out):
        if keep_k is not None and o > 0:
            gl = [g if k <= keep_k else g[:0] for k, g in enumerate(G, start=1)]
            mapping = np.concatenate([f + np.arange(len(g)) for f, g in zip(first, gl)]).astype(np.int64)
        else:
            gl, mapping = [g.copy() for g in G], None
        outs.append({"K": len(G), "sizes": [len(g) for g in gl], "groups": gl, "C": synth.wishart_covariance(n, o)[0],
                     "mapping": None if keep_k is None else (mapping if mapping is not None else np.arange(L, dtype=np.int64))})
        local.append(gl)
    rng = np.random.RandomState(8000 + i)
    has = lambda model: np.concatenate([(g == model).any(axis=1) for g in G])      # noqa: E731
    ok = 0.5 + rng.rand(L)
    allocs = {"ok": ok, "no3": ok * ~has(3), "no0": ok * ~has(0), "tiny2": np.where(has(2), 1.0e-7, ok)}
    return dict(n=n, L=L, outs=outs, groups=G, local=local, env=env, allocs=allocs, n_out=n_out)


def layout(p):
    """what layout_tiles and the dispatchers decide for problem p, restated: NT, KU, tile wavefronts of the instantiation, tiles
    per workgroup, workgroups per output (padded), bpo (0 when they differ)"""
    n, n_out = p["n"], p["n_out"]
    nt = pick(NT_SET, n)
    kmax = max(k for gl in p["local"] for k, g in enumerate(gl, start=1) if len(g))
    kmax_plan = len(p["groups"])                       # the plan takes K, the length of the size list, as its widest group
    ku = pick(KU_SET, kmax_plan)
    fused = 15 if nt <= 26 and ku <= 8 else 7
    tiles = [sum(-(-len(g) // 64) for g in gl) for gl in p["local"]]
    tpb = min(fused, max(1, -(-max(tiles) // max(1, CUS // n_out))))
    wgs = [max(1, -(-t // tpb)) for t in tiles]
    return dict(nt=nt, ku=ku, fused_tpb=fused, tiles_per_wg=tpb, wgs=wgs, bpo=wgs[0] if len(set(wgs)) == 1 else 0, kmax=kmax,
                extra_rows=nt - 16 if 16 < nt <= 32 else 0)


def masks(p, kind):
    """per output (mask1, mask2 at delta = 0) as lists of bools per model: touched by a group with |m| > 1e-6 / with m != 0"""
    m = p["allocs"][kind]
    G, n = p["groups"], p["n"]
    first = np.concatenate([[0], np.cumsum([len(g) for g in G])[:-1]])
    out = []
    for gl in p["local"]:
        am = np.zeros(n)
        for f, g_all, g in zip(first, G, gl):
            mm = m[f:f + len(g)]                       # (a local list is a prefix-by-size of the global one: same order)
            for j in range(g.shape[1]):
                np.maximum.at(am, g[:, j], np.abs(mm))
        out.append((am > 1.0e-6, am > 0.0))
    return out


def _bits(a):
    a = np.ascontiguousarray(a)
    return a.view(np.int64) if a.dtype == np.float64 else a


def record(plan, name, p, peek_v):
    """what the fixture holds of one case: {<name>/<call>/<what>: array}; doubles are stored as their int64 bit patterns, so
    that a NaN compares like any other value.  peek_v() returns the plan's v workspace (n_out * n doubles) after a launch."""
    import torch
    out = {}
    if name == "ma_n6_o1":
        return _record_ma(plan, name, p)
    for label, kind, delta, from_rec in CALLS:
        m = p["allocs"][kind]
        if from_rec:
            var, grad, st = plan.solve_grad(plan.phi(m), delta=delta)
        else:
            var, grad, st = plan.eval(m, delta=delta)
        torch.cuda.synchronize()
        for what, a in (("var", var.cpu().numpy()), ("grad", grad.cpu().numpy()), ("st", st.cpu().numpy()), ("v", peek_v())):
            out["%s/%s/%s" % (name, label, what)] = _bits(a)
    return out


def _record_ma(plan, name, p):
    import torch
    from bluest_amd._lib import check
    from bluest_amd.plan import _stream
    rng = np.random.RandomState(8100)
    L = p["L"]
    x0 = rng.rand(L) + 0.1
    x0 /= x0.sum()
    cc_h = 1.0 / (0.5 + rng.rand(L))
    up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(plan.device)      # noqa: E731
    x_d, m_d, cc, s_d = up(x0), up(cc_h * x0), up(cc_h), up(np.array([1.7]))
    var = torch.zeros((1, 1), dtype=torch.float64, device=plan.device)
    st = torch.zeros((1, 1), dtype=torch.int32, device=plan.device)
    out = {}
    for step in range(MA_STEPS):
        check(plan.lib.bluest_plan_eval_ma(plan._h, m_d.data_ptr(), var.data_ptr(), st.data_ptr(), s_d.data_ptr(), cc.data_ptr(),
                                           x_d.data_ptr(), _stream()))
        torch.cuda.synchronize()
        for what, a in (("x", x_d), ("m", m_d), ("var", var), ("st", st)):
            out["%s/step%d/%s" % (name, step, what)] = _bits(a.cpu().numpy())
    return out


def keys(name):
    if name == "ma_n6_o1":
        return ["%s/step%d/%s" % (name, s, w) for s in range(MA_STEPS) for w in ("x", "m", "var", "st")]
    return ["%s/%s/%s" % (name, c[0], w) for c in CALLS for w in ("var", "grad", "st", "v")]

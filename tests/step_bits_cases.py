"""
Plans and allocations of tests/test_gpu_step_bits.py, shared with tools/gen_golden_step_bits.py (which recorded
tests/golden/step_bits_parent.npz).  numpy only; every input is seeded, so the fixture holds results only.

Each case is the smallest plan that reaches one path of the evaluation kernels:
  shared_o3   n=8 / k_max=3 / 3 outputs     k_phi_chunks_shared<2>, the second block's clamped last output, regular fold
  plain_o1    the same, 1 output            k_phi_chunks, slot table
  shared_o8   the same, 8 outputs           36 chunks per output: far below the 4096 wavefronts a wider OB needs, so OB = 2
  rowrag_o2   rows of unequal chunk counts  descriptor fold (FoldReg.Cd == 0), shared kernel without a slot table
  rowrag_o1   the same, 1 output            plain kernel without a slot table
  cols32_o1   L_global = 70 000 + mapping   int32 columns
  long_o1     n=16, every subset            32 768 entries per diagonal row, above the 64 x 256 of iters = 1: iters = 2 (n=12 /
                                            k_max=12 has 2048 per row and stays at iters = 1), 64 chunks per diagonal row: the
                                            descriptor fold's second sweep.  Of its 65 535 gradient entries every 61st is recorded.
"""
import numpy as np

from bluest_amd import synth

CH0 = 256                     # entries per chunk and iteration (csrc/plan.hip)
GRAD_STRIDE = {"long_o1": 61}


def _all(n, kmax):
    return synth.all_groups(n, kmax)


def _rowrag_groups(n=11):
    """singletons, every pair, and every subset holding models 0 AND 1.  Entries per row: (0,0) and (1,1) 522 (three chunks),
    (0,1), (0,a), (1,a) and (a,a) 257..512 (two), (a,b) 129 (one) for a, b >= 2: fixed strides would waste a third of the slots"""
    by_k = {k: [] for k in range(1, n + 1)}
    for g in synth.all_groups(n, 2):
        by_k[g.shape[1]].extend(tuple(r) for r in g.tolist())
    for bits in range(1 << (n - 2)):
        g = (0, 1) + tuple(i + 2 for i in range(n - 2) if bits >> i & 1)
        if len(g) > 2:
            by_k[len(g)].append(g)
    return [np.array(sorted(by_k[k]), dtype=np.int64).reshape(-1, k) for k in range(1, n + 1)]


def row_chunks(n, groups):
    """(chunks per symmetric destination (a <= b), iters) as layout_phi chooses them: at most 64 chunks in the longest row"""
    cnt = np.zeros((n, n), dtype=np.int64)
    for g in groups:
        for j in range(g.shape[1]):
            for l in range(j, g.shape[1]):
                np.add.at(cnt, (np.minimum(g[:, j], g[:, l]), np.maximum(g[:, j], g[:, l])), 1)
    iters = 1
    while -(-int(cnt.max()) // (CH0 * iters)) > 64 and iters < 1024:
        iters *= 2
    return -(-cnt // (CH0 * iters)), iters


def regular_fold(n, groups, n_out):
    """layout_fold_reg's decision: fixed strides per destination class when that wastes at most a quarter of the slots"""
    ch, _ = row_chunks(n, groups)
    iu = np.triu_indices(n, 1)
    Cd, Co = int(np.diag(ch).max()), max(int(ch[iu].max()), 1)
    slots = n * Cd + len(iu[0]) * Co
    n_chunks = int(np.diag(ch).sum() + ch[iu].sum()) * n_out
    return Cd <= 32 and Co <= 32 and slots * n_out * 4 <= n_chunks * 5


#        name         n   groups                 n_out  L_global  expect (launch_config keys)
CASES = [
    ("shared_o3", 8, lambda: _all(8, 3), 3, None, dict(phi_ob=2, cols16=1, iters=1, path=1)),
    ("plain_o1", 8, lambda: _all(8, 3), 1, None, dict(phi_ob=0, cols16=1, iters=1, path=1)),
    ("shared_o8", 8, lambda: _all(8, 3), 8, None, dict(phi_ob=2, cols16=1, iters=1, path=1)),
    ("rowrag_o2", 11, _rowrag_groups, 2, None, dict(phi_ob=2, cols16=1, iters=1, path=1)),
    ("rowrag_o1", 11, _rowrag_groups, 1, None, dict(phi_ob=0, cols16=1, iters=1, path=1)),
    ("cols32_o1", 8, lambda: _all(8, 3), 1, 70000, dict(phi_ob=0, cols16=0, iters=1, path=1)),
    ("long_o1", 16, lambda: _all(16, 16), 1, None, dict(phi_ob=0, cols16=1, iters=2, path=1)),
]
NAMES = [c[0] for c in CASES]


def problem(name):
    """(n, L_global, outputs for Plan(), m1 (L_global,), M2 (2, L_global), expected launch configuration, regular fold?)"""
    _, n, mk, n_out, Lg, expect = CASES[NAMES.index(name)]
    groups = mk()
    L = int(sum(len(g) for g in groups))
    rng = np.random.RandomState(4000 + NAMES.index(name))
    mapping = None
    if Lg is not None:
        mapping = np.sort(rng.choice(Lg, L, replace=False)).astype(np.int64)
        mapping[-1] = Lg - 1                                  # a column index above 65 535 is really stored
    else:
        Lg = L
    outs = [{"K": len(groups), "sizes": [len(g) for g in groups], "groups": [g.copy() for g in groups],
             "C": synth.wishart_covariance(n, o)[0], "mapping": mapping} for o in range(n_out)]
    m1 = 10.0 * rng.rand(Lg)
    M2 = np.stack([0.5 + rng.rand(Lg), (0.5 + rng.rand(Lg)) * (rng.rand(Lg) < 0.6)])
    if mapping is not None:
        M2[1, mapping[:n]] = 0.75                             # the singletons stay sampled
    else:
        M2[1, :n] = 0.75
    return n, Lg, outs, m1, M2, expect, regular_fold(n, groups, n_out)


def record(plan, name, m1, M2):
    """what the fixture holds of one case: host arrays keyed <name>/<what>"""
    s = GRAD_STRIDE.get(name, 1)
    out = {}
    out["phi1"] = plan.phi(m1).cpu().numpy()
    v, g, st = plan.eval(m1)
    out["var1"], out["grad1"], out["st1"] = v.cpu().numpy(), g.cpu().numpy()[:, ::s].copy(), st.cpu().numpy()
    out["phi2"] = plan.phi(M2).cpu().numpy()
    v, g, st = plan.eval(M2)
    out["var2"], out["grad2"], out["st2"] = v.cpu().numpy(), g.cpu().numpy()[:, ::s].copy(), st.cpu().numpy()
    return {"%s/%s" % (name, k): a for k, a in out.items()}

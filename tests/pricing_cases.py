"""
Case table of the pricing / support-point / multiplicative-update tests (test_pricing_ref.py on the CPU, test_gpu_pricing.py on
the GPU): plan shapes, synthetic inputs with planted maxima and ties, and their references (oracle/pricing_ref.py).

A shape is (plan key, n_out, ragged).  Its inputs are per-group quadratic forms q[o][i] >= 0 (the gradient handed to the
kernels is grad[goff[o] + li] = -q[o][mapping_o[li]], every other entry of the buffer poisoned), multipliers mu, scales s and
the factors cc.  A case patches single columns of the shape's base inputs: a planted maximum multiplies column i by a power of
two, a tie copies column i to column j bit for bit (q, cc and the cap mask; i and j belong to the same outputs).  A reduced
cost depends on its own column only, so the reference of a case recomputes the patched columns and keeps the others.

Every buffer a kernel receives has its documented size, every support index is in [0, L) and ascending, and no cap mask has a
bit at or above the number of caps; nu always holds 64 entries.
"""
import numpy as np

from bluest_amd import synth
from oracle import pricing_ref as ref

PLANS = {"n4": (4, 2), "n6": (6, 3), "n12": (12, 4), "n20": (20, 5)}          # L = 10, 41, 793, 21 699
PRICE_SHAPES = [(p, n_out, ragged) for p in ("n6", "n12", "n20") for n_out, ragged in ((1, False), (3, False), (3, True))] + [("n4", 3, False)]
POISON = -1.0e300          # unread gradient entries: one of them read would be the largest reduced cost by far
STRIDE, THREADS = ref.PRICE_STRIDE, ref.PRICE_THREADS

_shapes, _base = {}, {}


def block_of(i): return (i % STRIDE) // THREADS
def thread_of(i): return i % THREADS
def wave_of(i): return thread_of(i) // 64


def shape(key, n_out, ragged):
    """host description of one plan: groups, the outputs as plan.Plan takes them (built as test_gpu_launch_matrix._problem does:
    every singleton, about 70 % of the other groups per output), the local -> global mappings and their inverse"""
    k_ = (key, n_out, ragged)
    if k_ in _shapes:
        return _shapes[k_]
    n, K = PLANS[key]
    rng = np.random.RandomState(1000 * n + 10 * n_out + ragged)
    G = synth.all_groups(n, K)
    sizes = np.array([len(g) for g in G])
    L = int(sizes.sum())
    first = np.concatenate([[0], np.cumsum(sizes)[:-1]])
    outs, mappings = [], []
    for o in range(n_out):
        keep = [np.ones(len(g), bool) if (k == 1 or not ragged) else rng.rand(len(g)) < 0.7 for k, g in enumerate(G, start=1)]
        mapping = np.concatenate([f + np.flatnonzero(kk) for f, kk in zip(first, keep)]).astype(np.int64)
        gl = [g[kk] for g, kk in zip(G, keep)]
        outs.append({"K": K, "sizes": [len(g) for g in gl], "groups": gl, "C": synth.wishart_covariance(n, o)[0],
                     "mapping": mapping if ragged else None})
        mappings.append(mapping)
    invmap = None
    if ragged:
        invmap = np.full((n_out, L), -1, dtype=np.int32)
        for o, mp in enumerate(mappings):
            invmap[o, mp] = np.arange(len(mp), dtype=np.int32)
    sh = dict(key=key, n=n, K=K, L=L, n_out=n_out, ragged=ragged, outs=outs, mappings=mappings, invmap=invmap,
              lens=[len(mp) for mp in mappings], name="%s_o%d%s" % (key, n_out, "_ragged" if ragged else ""))
    sh["goff_host"] = [int(x) for x in np.concatenate([[0], np.cumsum(sh["lens"])[:-1]])]
    sh["grad_len_host"] = int(sum(sh["lens"]))
    present = np.ones((n_out, L), bool) if invmap is None else invmap >= 0
    sh["pattern"] = present.T.astype(np.int64) @ (1 << np.arange(n_out, dtype=np.int64))      # bit o: group i belongs to output o
    _shapes[k_] = sh
    return sh


def base_inputs(sh):
    """the shape's unpatched inputs (shared, read-only)"""
    if sh["name"] not in _base:
        rng = np.random.RandomState(7 + sh["L"] + sh["n_out"] + sh["ragged"])
        L, n_out, N = sh["L"], sh["n_out"], sh["n"]
        mu = rng.rand(n_out) + 0.2
        b = dict(q=0.5 + rng.rand(n_out, L), cc=0.5 + 1.5 * rng.rand(L), mu=mu / mu.sum(),
                 s=1.0 + 0.3 * rng.rand(n_out) if n_out > 1 else np.array([0.37]), v_ws=1.0 + rng.rand(n_out * N),
                 mask64=rng.randint(0, 1 << 62, size=L).astype(np.uint64) << np.uint64(2) | rng.randint(0, 4, size=L).astype(np.uint64),
                 nu64=0.05 * rng.rand(64), F=1.0 + rng.rand())
        b["mask64"][rng.rand(L) < 0.3] = 0                          # groups without a capped model
        b["mask64"][L - 1] |= np.uint64(1) << np.uint64(63)         # bit 63 is used
        for a in b.values():
            if isinstance(a, np.ndarray):
                a.setflags(write=False)
        _base[sh["name"]] = b
    return _base[sh["name"]]


def support(sh):
    """ascending support: group 0, group L-1, (ragged) a group absent from output 1, the rest spread over [0, L)"""
    L = sh["L"]
    S = min(64, max(1, L // 2))
    sup = set(int(x) for x in np.linspace(0, L - 1, S).astype(np.int64))
    if sh["ragged"]:
        absent = np.flatnonzero(sh["invmap"][1] < 0)
        sup.discard(sorted(sup)[1])
        sup.add(int(absent[len(absent) // 2]))
    return np.array(sorted(sup), dtype=np.int64)


def _same_pattern(sh, i, ok):
    """the first j > i of the same output pattern as group i for which ok(j)"""
    for j in range(i + 1, sh["L"]):
        if sh["pattern"][j] == sh["pattern"][i] and ok(j):
            return j
    raise AssertionError("no partner for group %d in %s" % (i, sh["name"]))


def _member(sh, start):
    """the first group >= start that belongs to at least one output whose multiplier the cases keep positive (output 0)"""
    i = start
    while not (sh["pattern"][i] & 1):
        i += 1
    return i


def _stride_pair(sh, start):
    """the first i >= start such that groups i and i + STRIDE (one thread's first and second round) have one output pattern"""
    i = _member(sh, start)
    while sh["pattern"][i + STRIDE] != sh["pattern"][i]:
        i = _member(sh, i + 1)
    return i


def tie_pairs(sh):
    """[(kind, i, j, factor)]: j receives column i bit for bit; both are then multiplied by `factor` (distinct powers of two, so that
    the pairs do not tie with one another and lead their workgroups)"""
    L, out = sh["L"], []
    i = _member(sh, 3)
    out.append(("wave", i, _same_pattern(sh, i, lambda j: block_of(j) == block_of(i) and wave_of(j) == wave_of(i)), 64.0))
    if L > 256:
        i = _member(sh, 70)
        out.append(("waves", i, _same_pattern(sh, i, lambda j: block_of(j) == block_of(i) and wave_of(j) != wave_of(i)), 128.0))
        i = _member(sh, 300)
        out.append(("workgroups", i, _same_pattern(sh, i, lambda j: block_of(j) != block_of(i)), 256.0))
    if L > STRIDE:
        i = _stride_pair(sh, 1000)
        out.append(("stride", i, i + STRIDE, 512.0))                # one thread meets both: it keeps the first
        if sh["pattern"][STRIDE - 1] == sh["pattern"][STRIDE] and sh["pattern"][STRIDE] & 1:
            out.append(("rounds", STRIDE - 1, STRIDE, 1024.0))      # the global maximum twice: last thread of round 0, first of round 1
    return out


def price_cases(sh):
    """the synthetic pricing cases of one shape: dicts name, sh, patches [(i, source column, factor)], caps (0, 3, 64), inf
    (output 1 has mu = 0 and an infinite gradient), expect (what the table test must find in the reference)"""
    L, n_out = sh["L"], sh["n_out"]
    mk = lambda name, patches=(), caps=0, inf=False, **expect: dict(name="%s-%s" % (sh["name"], name), sh=sh, patches=list(patches),   # noqa: E731
                                                                    caps=caps, inf=inf, expect=expect)
    ties = [p for _, i, j, f in tie_pairs(sh) for p in ((i, i, f), (j, i, f))]
    cases = [mk("base"), mk("ties", ties, ties=tie_pairs(sh))]
    for i in [0, L - 1] + ([STRIDE - 1, STRIDE] if L > STRIDE else []):
        if sh["pattern"][i] & 1:
            cases.append(mk("max_at_%d" % i, [(i, i, 4096.0)], argmax=i))
    if L > STRIDE:
        i = _stride_pair(sh, 7)
        cases.append(mk("stride_pair", [(i, i, 1024.0), (i + STRIDE, i + STRIDE, 2048.0)], stride_pair=(i, i + STRIDE)))
    cases += [mk("caps3", ties, caps=3, ties=tie_pairs(sh)), mk("caps64", ties, caps=64, ties=tie_pairs(sh), negative=True)]
    if n_out == 3 and L < STRIDE:
        cases.append(mk("inf_gradient", ties, inf=True))
    return cases


def all_price_cases():
    return [c for key, n_out, ragged in PRICE_SHAPES for c in price_cases(shape(key, n_out, ragged))]


def inputs(case, goff=None, grad_len=None):
    """the arrays of one call, as the kernel takes them (host copies): grad, mu, s, cc, sup, v_ws, capmask / nu / master_out
    (None without caps), and q.  goff / grad_len: the plan's gradient layout (default: the outputs back to back)"""
    sh, b = case["sh"], base_inputs(case["sh"])
    goff = sh["goff_host"] if goff is None else [int(x) for x in goff]
    grad_len = sh["grad_len_host"] if grad_len is None else int(grad_len)
    q, cc, mu = b["q"].copy(), b["cc"].copy(), b["mu"].copy()
    mask = None
    if case["caps"]:
        mask = b["mask64"] & np.uint64((1 << case["caps"]) - 1) if case["caps"] < 64 else b["mask64"].copy()
    for i, src, f in case["patches"]:
        q[:, i], cc[i] = b["q"][:, src] * f, b["cc"][src]
        if mask is not None:
            mask[i] = mask[src]
    if case["inf"]:
        mu[1], q[1, :] = 0.0, np.inf
    grad = np.full(grad_len, POISON)
    for o, mp in enumerate(sh["mappings"]):
        assert goff[o] >= 0 and goff[o] + len(mp) <= grad_len
        grad[goff[o]:goff[o] + len(mp)] = -q[o, mp]
    nu = master_out = None
    if case["caps"]:
        nu = np.full(64, np.nan)                                    # entries at and above the number of caps are never read
        nu[:case["caps"]] = b["nu64"][:case["caps"]] * (64.0 / case["caps"])
        master_out = np.concatenate([[b["F"]], np.full(15 + sh["n_out"], np.nan)])
    return dict(grad=grad, goff=goff, mu=mu, s=b["s"].copy(), cc=cc, sup=support(sh), v_ws=b["v_ws"].copy(), capmask=mask, nu=nu,
                master_out=master_out, q=q)


_c0 = {}


def _uncapped(case, a):
    """reduced costs without the cap correction: the shape's base ones, the patched columns recomputed"""
    sh = case["sh"]
    args = (sh["n_out"], a["grad"], a["goff"], sh["invmap"], list(a["mu"]), list(a["s"]), list(a["cc"]))
    if case["inf"]:
        return np.array([ref.reduced_cost(i, *args) for i in range(sh["L"])])
    key = (sh["name"], tuple(a["goff"]))
    if key not in _c0:
        a0 = inputs(dict(case, patches=[], caps=0), a["goff"], len(a["grad"]))
        args0 = (sh["n_out"], a0["grad"], a0["goff"], sh["invmap"], list(a0["mu"]), list(a0["s"]), list(a0["cc"]))
        _c0[key] = np.array([ref.reduced_cost(i, *args0) for i in range(sh["L"])])
        _c0[key].setflags(write=False)
    c = _c0[key].copy()
    for i in set(p[0] for p in case["patches"]):
        c[i] = ref.reduced_cost(i, *args)
    return c


def reference(case, a):
    """what bluest_price / bluest_price_capped must write for the inputs `a` of `case` (as ref.price returns it)"""
    sh = case["sh"]
    c = _uncapped(case, a)
    if case["caps"]:
        F2 = float(a["master_out"][0]) * float(a["master_out"][0])
        for i in range(sh["L"]):
            mk, corr, bit = int(a["capmask"][i]), 0.0, 0
            while mk:
                if mk & 1:
                    corr = corr + float(a["nu"][bit])
                mk >>= 1
                bit += 1
            c[i] = ref.fma(-float(a["cc"][i]) * F2, corr, float(c[i]))
    top_val, top_idx = ref.report(c)
    return {"c": c, "c_sup": c[a["sup"]].copy(), "top_val": top_val, "top_idx": top_idx,
            "y0": np.array([a["v_ws"][o * sh["n"]] for o in range(sh["n_out"])])}


# ---- multiplicative update -------------------------------------------------------------------------------
MA_SHAPES = [("n6", 1, False), ("n12", 3, False), ("n12", 3, True), ("n6", 9, False), ("n6", 9, True), ("n4", 64, False), ("n4", 64, True),
             ("n20", 3, True)]


def ma_inputs(sh, p, goff=None, grad_len=None, fault=None):
    """var, status, grad (every term of one sign: q > 0), s, cc, x, m of one bluest_ma_update call; fault: None, "status" (one
    status not OK), "inf" (r_max infinite), "zero" (r_max 0)"""
    L, n_out = sh["L"], sh["n_out"]
    rng = np.random.RandomState(99 + L + n_out + sh["ragged"])
    case = dict(sh=sh, patches=[], caps=0, inf=False)
    a = inputs(case, goff, grad_len)
    var = 0.5 + rng.rand(n_out)
    status = np.zeros(n_out, dtype=np.int32)
    if fault == "status":
        status[n_out - 1] = 3
    elif fault == "inf":
        var[n_out // 2] = np.inf
    elif fault == "zero":
        var[:] = 0.0
    x = rng.rand(L) + 0.1
    x /= x.sum()
    return dict(var=var, status=status, grad=a["grad"], goff=a["goff"], s=a["s"], cc=a["cc"], p=float(p), x=x, m=a["cc"] * x)


def ma_reference(sh, a):
    return ref.ma_update(sh["L"], sh["n_out"], a["var"], a["status"], a["grad"], a["goff"], sh["invmap"], a["s"], a["cc"], a["p"], a["x"], a["m"])


def ma_bound(n_out):
    """relative bound on x and m for p != 1 (all terms of one sign, so every sum is as accurate as its terms): den and num are
    n_out-term fma chains of products with a weight that carries the pow error and one division, (n_out + 2 + U) eps each;
    three more operations give x, one more m"""
    return (2 * n_out + 6 + 2 * ref.POW_ULPS) * ref.DBL_EPS


# ---- support point ----------------------------------------------------------------------------------------
def support_cases():
    """(name, L, S, sup, xs, cc, eps): S = 1 and S = 64, first and last group in the support"""
    out = []
    for L, S in ((41, 1), (793, 64), (21699, 64), (793, 1)):
        rng = np.random.RandomState(L + S)
        if S == 1:
            sups = [np.array([0], dtype=np.int64), np.array([L - 1], dtype=np.int64)]
        else:
            mid = np.sort(rng.choice(np.arange(1, L - 1), S - 2, replace=False))
            sups = [np.concatenate([[0], mid, [L - 1]]).astype(np.int64)]
        for sup in sups:
            xs = rng.rand(S) + 0.1
            xs /= xs.sum()
            for eps in (0.0, 1e-6, 1e-3):
                out.append(("L%d_S%d_first%d_eps%g" % (L, S, sup[0], eps), L, S, sup, xs, 0.5 + 1.5 * rng.rand(L), eps))
    return out

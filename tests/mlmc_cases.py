"""
The inputs of the MLMC subset-search tests at the kernel's interface (bluest_mlmc_search), shared by the CPU tests of the
restatement (test_mlmc_ref.py: the table covers the intended paths) and the GPU tests (test_gpu_mlmc_search.py: the kernel equals
the restatement).  Each case is the smallest input that drives one path of csrc/mlmc.hip; `group` names the path.
"""
import numpy as np

import mlmc_ref as ref

EPS, BUDGET, EPS_CONT, BUDGET_CONT = 0, ref.BUDGET, ref.CONTINUOUS, ref.BUDGET | ref.CONTINUOUS
MODES = {"eps": EPS, "budget": BUDGET, "eps_cont": EPS_CONT, "budget_cont": BUDGET_CONT}


def complete(nb):
    return np.array([((2 << nb) - 1) & ~(1 << p) for p in range(nb + 1)], dtype=np.uint32)


def chain(nb):
    return np.array([sum(1 << q for q in (p - 1, p + 1) if 0 <= q <= nb) for p in range(nb + 1)], dtype=np.uint32)


def blocks(nb):
    """position 0 coupled to all; positions 1..nb coupled inside blocks of 6 (counted from the cheap end) with |p - q| <= 2"""
    blk = lambda p: (nb - p) // 6
    adj = [sum(1 << q for q in range(1, nb + 1))]
    for p in range(1, nb + 1):
        adj.append(1 | sum(1 << q for q in range(1, nb + 1) if q != p and blk(q) == blk(p) and abs(p - q) <= 2))
    return np.array(adj, dtype=np.uint32)


def case(name, group, flags, w, lv, adj, budget=0.0, eps=None, rc=ref.RC_OK, **extra):
    lv = np.asarray(lv, dtype=np.float64)
    if lv.ndim == 2: lv = lv[None]
    n_out, nb = lv.shape[0], lv.shape[1] - 1
    eps = None if eps is None else np.broadcast_to(np.asarray(eps, dtype=np.float64), (n_out,)).copy()
    args = dict(nb=nb, n_out=n_out, flags=flags, budget=float(budget), eps2=None if eps is None else eps**2,
                w=np.asarray(w, dtype=np.float64), lv=np.ascontiguousarray(lv), adj=np.asarray(adj, dtype=np.uint32))
    d = dict(name=name, group=group, args=args, rc=rc)
    d.update(extra)
    return d


def table(tail):
    """level variances of a telescoping hierarchy with Var(model p) = tail[p]: lv[p][q] = tail[p] + (tail[q] - 2 tail[q])"""
    n = len(tail)
    lv = np.full((n, n), np.nan)
    for p in range(n):
        lv[p, p] = tail[p]
        for q in range(p + 1, n): lv[p, q] = tail[p] + (tail[q] - 2 * tail[q])
    return lv


def hierarchy(nb, n_out, seed, rate=4.0, cost=2.0):
    """the telescoping hierarchy of tools/gen_golden_mlmc.py by position: (w, lv, rng)"""
    rng = np.random.RandomState(seed)
    n = nb + 1
    lv = []
    for o in range(n_out):
        var = rate ** (-(n - 1 - np.arange(n)) * (1 + 0.25 * o / max(n_out - 1, 1))) * rng.uniform(0.8, 1.25, n)
        lv.append(table(np.cumsum(var[::-1])[::-1]))
    w = np.sort(cost ** (-np.arange(n, dtype=np.float64)) * rng.uniform(0.95, 1.05, n))[::-1].copy()
    w[0] = w[0] * 1.01
    return w, np.array(lv), rng


def _mode_kw(mode, w, lv, rng, tol=0.01, many=317.3):
    if MODES[mode] & BUDGET: return dict(budget=many * w[0])
    return dict(eps=tol * np.sqrt(lv[:, 0, 0]) * rng.uniform(0.9, 1.1, lv.shape[0]))


def base_cases():
    out = []
    for n_out in (1, 3, 64):
        for nb in (0, 1, 2, 7):
            for mode, flags in MODES.items():
                w, lv, rng = hierarchy(nb, n_out, 100 * n_out + nb)
                out.append(case("base_%s_nb%d_out%d" % (mode, nb, n_out), "base", flags, w, lv, complete(nb),
                                **_mode_kw(mode, w, lv, rng)))
    return out


def veto_cases():
    """output 1 alone has a NaN level variance on the first pair of the group that wins without it"""
    out = []
    for mode in ("eps", "budget", "eps_cont", "budget_cont"):
        w, lv, rng = hierarchy(7, 3, 707)
        kw = _mode_kw(mode, w, lv, rng)
        plain = case("veto_%s_plain" % mode, "veto_plain", MODES[mode], w, lv, complete(7), **kw)
        first = (reference(plain).best_mask & -reference(plain).best_mask).bit_length()      # g_1 of the plain winner
        lv = lv.copy()
        lv[1, 0, first] = np.nan
        out += [plain, case("veto_%s" % mode, "veto", MODES[mode], w, lv, complete(7), plain=plain["name"], pair=(0, first), **kw)]
    return out


def graph_cases():
    """nb = 21 and 30, sparse: 46 paths per full block of 6.  The blocks repeat one hierarchy; every block but the cheapest is
    far from model 0 (its first level is large), so the winner lies in the cheapest block and keeps a bit at or above 20"""
    out = []
    for nb in (21, 30):
        for n_out in (1, 3):
            rng = np.random.RandomState(nb + n_out)
            p = np.arange(nb + 1)
            h = np.where(p == 0, 0, 1 + (p - 1 - (nb - 6)) % 6)                 # place in the block's hierarchy, 1..6
            blk = np.where(p == 0, 0, (nb - p) // 6)                            # 0 = cheapest block
            w = 2.0 ** (-h.astype(np.float64)) * 1.5 ** blk * rng.uniform(0.97, 1.03, nb + 1)
            w[h == 6] *= 0.25                                                   # the last of a block is cheap: the winner ends in it
            w[0] = 1.3 * w.max()
            lv = []
            for o in range(n_out):
                var = 4.0 ** (-(6 - np.arange(7)) * (1 + 0.1 * o)) * rng.uniform(0.8, 1.25, 7)
                tail = np.cumsum(var[::-1])[::-1][h] * rng.uniform(0.999, 1.001, nb + 1)
                t = np.abs(tail[:, None] - tail[None, :])
                t[0, blk > 0] += 0.05 * tail[0]
                np.fill_diagonal(t, tail)
                lv.append(t)
            lv = np.array(lv)
            for mode in ("eps", "budget"):
                out.append(case("graph_%s_nb%d_out%d" % (mode, nb, n_out), "graph", MODES[mode], w, lv, blocks(nb),
                                **_mode_kw(mode, w, lv, rng, tol=0.013, many=291.7)))
    return out


def flat(nb, n_out, seed):
    """model 0 = Z + a E_0, model j = Z + tiny E_j with costs a thousand times below model 0's: every group has the same first
    level (variance 0.01, cost about 1) and a last level of variance 1; the levels between have almost no variance and clamp
    to one sample.  With one or two samples on the first level the all-floor and all-ceil objectives of every group straddle
    every other group's, so all 2^nb groups are candidates; the small terms tell them apart."""
    rng = np.random.RandomState(seed)
    w = np.concatenate([[1.0], np.sort(1e-3 * 2.0 ** (-np.arange(nb) / 2.0) * rng.uniform(0.97, 1.03, nb))[::-1]])
    lv = []
    for o in range(n_out):
        s = np.concatenate([[0.01 * (1 + 0.2 * o)], 1e-9 * rng.uniform(0.5, 2.0, nb)])
        t = s[:, None] + s[None, :]
        np.fill_diagonal(t, 1.0 + s)
        lv.append(t)
    return w, np.array(lv)


def window_cases():
    """nb = 17, complete: 2^17 groups, more than CAND_CAP of them candidates, so the host loop bisects its windows.  The
    tolerance is loose: the first level takes one or two samples, the levels between clamp to one, only the last rounds."""
    w, lv = flat(17, 2, 17)
    return [case("window_eps_out1", "window", EPS, w, lv[:1], complete(17), eps=0.1),
            case("window_eps_out2", "window", EPS, w, lv, complete(17), eps=[0.1, 0.107]),
            case("window_budget_out1", "window", BUDGET, w, lv[:1], complete(17), budget=1.6)]


def tie_cases():
    """same size: position 6 is a bit-identical copy of position 5 (cost, variances; a level between the two is as bad as a last
    level, so no good group holds both), so a group with one ties with the same group with the other, and the one that removes
    the lower position comes first.
    Different sizes: position nb is a ghost -- a model of variance 0 and a cost that vanishes in every sum, whose difference to
    any model z has the variance of z -- so a group and the same group with the ghost appended tie, and the larger comes first."""
    out = []
    for mode in MODES:
        w, lv, rng = hierarchy(6, 2, 60)
        kw = _mode_kw(mode, w, lv, rng)
        w, lv = w.copy(), lv.copy()
        w[6] = w[5]
        lv[:, :, 6], lv[:, 6, 6], lv[:, 5, 6] = lv[:, :, 5], lv[:, 5, 5], lv[:, 5, 5]
        out.append(case("tie_same_size_%s" % mode, "tie", MODES[mode], w, lv, complete(6), tie="same", **kw))
        w, lv, rng = hierarchy(5, 2, 61)
        kw = _mode_kw(mode, w, lv, rng)
        w = np.concatenate([w, [1.3e-30 * w[0]]])
        big = np.full((2, 7, 7), np.nan)
        big[:, :6, :6] = lv
        for z in range(6): big[:, z, 6] = lv[:, z, z]
        big[:, 6, 6] = 0.0
        out.append(case("tie_sizes_%s" % mode, "tie", MODES[mode], w, big, complete(6), tie="sizes", **kw))
    return out


def status_cases():
    w, lv, _ = hierarchy(3, 1, 5)
    out = [case("none_budget_below_w0", "status", BUDGET, w, lv, complete(3), budget=0.93 * w[0])]
    w, lv, _ = hierarchy(25, 1, 25, rate=1.7, cost=1.5)
    out.append(case("too_big", "status", EPS, w, lv, chain(25), eps=1e-3))
    out.append(case("too_big_budget", "status", BUDGET, w, lv, chain(25), budget=1e6 * w[0]))
    out.append(case("too_big_input_continuous", "status", EPS_CONT, w, lv, chain(25), eps=1e-3))
    return out


def arg_cases():
    """(name, changes to a valid call) -- each must return BLUEST_ERR_ARG before any launch"""
    return [("nb_31", dict(nb=31)), ("nb_negative", dict(nb=-1)), ("n_out_0", dict(n_out=0)), ("n_out_65", dict(n_out=65)),
            ("eps_mode_without_eps2", dict(eps2=None)), ("null_w", dict(w=None)), ("null_lv", dict(lv=None)),
            ("null_adj", dict(adj=None)), ("null_output", dict(outputs_given=False))]


def valid_small():
    w, lv, rng = hierarchy(2, 1, 3)
    return case("valid_small", "base", EPS, w, lv, complete(2), eps=0.013 * np.sqrt(lv[0, 0, 0]))


_RESULTS = {}


def reference(c):
    """the restatement's answer for a case, computed once per process and shared"""
    if c["name"] not in _RESULTS:
        _RESULTS[c["name"]] = ref.search(**c["args"])
    return _RESULTS[c["name"]]


def all_cases():
    return base_cases() + veto_cases() + graph_cases() + window_cases() + tie_cases() + status_cases()

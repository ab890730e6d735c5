"""
The inputs of the MFMC subset-search tests at the kernel's interface (bluest_mfmc_search), shared by the CPU tests of the
reference (test_mfmc_ref.py: every case is sound and the table covers the intended paths) and the GPU tests
(test_gpu_mfmc_search.py: the kernel equals the reference).  Each case is the smallest input that drives one path of
csrc/mfmc.hip; `group` names the path, `tie` marks the cases whose best objective is deliberately shared by two cliques.
"""
import numpy as np

from oracle import mfmc_ref as ref

EPS, BUDGET, EPS_CONT, BUDGET_CONT, SMALL = 0, ref.BUDGET, ref.CONTINUOUS, ref.BUDGET | ref.CONTINUOUS, ref.BUDGET | ref.SMALL_BUDGET
MODES = {"eps": EPS, "budget": BUDGET, "eps_cont": EPS_CONT, "budget_cont": BUDGET_CONT, "small_budget": SMALL}


def complete(nb):
    return np.array([((1 << nb) - 1) & ~(1 << b) for b in range(nb)], dtype=np.uint32)


def band(nb, width):
    """neighbours b, c adjacent iff |b - c| < width: overlapping blocks of `width`, about nb 2^(width-1) cliques"""
    return np.array([sum(1 << c for c in range(nb) if c != b and abs(b - c) < width) for b in range(nb)], dtype=np.uint32)


def order(rho):
    return np.array([np.argsort(np.abs(r), kind="stable")[::-1] for r in np.atleast_2d(rho)], dtype=np.int32)


def case(name, group, flags, w, s, rho, adj, budget=0.0, eps=None, perm=None, tie=False, rc=ref.RC_OK, **extra):
    s, rho = np.atleast_2d(np.asarray(s, dtype=np.float64)), np.atleast_2d(np.asarray(rho, dtype=np.float64))
    n_out, nb = rho.shape[0], rho.shape[1] - 1
    eps = None if eps is None else np.broadcast_to(np.asarray(eps, dtype=np.float64), (n_out,)).copy()
    args = dict(nb=nb, n_out=n_out, flags=flags, budget=float(budget), eps2=None if eps is None else eps**2,
                epsm2=None if eps is None else eps**-2, w=np.asarray(w, dtype=np.float64), s=np.ascontiguousarray(s),
                rho=np.ascontiguousarray(rho), perm=order(rho) if perm is None else np.asarray(perm, dtype=np.int32),
                adj=None if nb == 0 else np.asarray(adj, dtype=np.uint32))
    d = dict(name=name, group=group, args=args, tie=tie, rc=rc)
    d.update(extra)
    return d


def hierarchy(nb, n_out, seed, decay=0.02, span=4.0):
    """a generic model hierarchy: |rho| and cost fall with the index; output o raises the correlations to 1 + 0.3 o / n_out
    (the same order for every output) and has deviations and tolerances of its own"""
    rng = np.random.RandomState(seed)
    n = nb + 1
    a = np.concatenate([[1.0], np.clip(1 - decay * np.cumsum(rng.uniform(0.2, 1.0, nb)), 0.05, 1.0)])
    w = 10.0 ** (3 - span * np.arange(n) / max(nb, 1)) * rng.uniform(0.9, 1.1, n)
    w[0] = w.max() * 1.01
    rho = np.array([a ** (1 + 0.3 * o / n_out) for o in range(n_out)])
    s = rng.uniform(0.5, 2.0, (n_out, n))
    return w, s, rho, rng


def base_cases():
    out = []
    for n_out in (1, 3, 64):
        for nb in (0, 1, 2, 7):
            w, s, rho, rng = hierarchy(nb, n_out, 100 * n_out + nb)
            eps = s[:, 0] * rng.uniform(0.08, 0.12, n_out)
            for mode, flags in MODES.items():
                budget = (3.37 if mode == "small_budget" else 31.73) * w[0]
                out.append(case("base_%s_nb%d_out%d" % (mode, nb, n_out), "base", flags, w, s, rho, complete(nb),
                                budget=budget if flags & BUDGET else 0.0, eps=None if flags & BUDGET else eps))
    # two outputs that order models 1 and 2 differently by |rho| (setup_mfmc refuses the answer; the kernel computes it)
    w = np.array([1.0, 0.01, 0.008])
    for mode in ("eps", "budget"):
        out.append(case("base_%s_orders_differ" % mode, "base", MODES[mode], w, [[1, 1, 1], [1, 1.5, 0.7]],
                        [[1, 0.99, 0.97], [1, 0.97, 0.99]], complete(2), budget=103.7 if mode == "budget" else 0.0,
                        eps=None if mode == "budget" else [0.0103, 0.0097], orders_differ=True))
    # output 1 alone makes every clique with models 3 and 4 infeasible (its rho_3 and rho_4 nearly coincide)
    w, s, rho, rng = hierarchy(4, 3, 7, decay=0.01)
    rho[1, 4] = rho[1, 3] * (1 - 1e-4)
    for mode in ("eps", "budget"):
        out.append(case("base_%s_one_output_vetoes" % mode, "base", MODES[mode], w, s, rho, complete(4),
                        budget=31.17 * w[0] if mode == "budget" else 0.0, eps=None if mode == "budget" else 0.113 * s[:, 0],
                        veto_output=1))
    return out


def wide_inputs(nb, n_out, seed):
    """nb neighbours in overlapping blocks of 7 (band graph).  Each block of 7 indices is a hierarchy of its own (|rho| and
    cost falling with the index); every block below the top one is less correlated and dearer, so the best clique lies
    in the top block and ends in the cheapest model, neighbour nb - 1"""
    rng = np.random.RandomState(seed)
    b = np.arange(nb)
    h = (b - (nb - 7)) % 7                                  # place in the block's hierarchy
    blk = (nb - 1 - b) // 7                                 # 0 = top block
    a = 0.9995 ** ((h + 1.0) ** 2 * 4) * 0.97 ** blk * rng.uniform(0.999, 1.0, nb)
    w = 10.0 ** (-0.6 * (h + 1)) * 3.0 ** blk * rng.uniform(0.95, 1.05, nb)
    rho = np.array([np.concatenate([[1.0], a ** (1 + 0.2 * o)]) for o in range(n_out)])
    s = rng.uniform(0.5, 2.0, (n_out, nb + 1))
    return np.concatenate([[1.0], w]), s, rho


def wide_cases():
    out = []
    for nb in (21, 24, 30):
        for n_out in (1, 3):
            w, s, rho = wide_inputs(nb, n_out, nb + n_out)
            for mode in ("eps", "budget"):
                out.append(case("wide_%s_nb%d_out%d" % (mode, nb, n_out), "wide", MODES[mode], w, s, rho, band(nb, 7),
                                budget=29.33 if mode == "budget" else 0.0,
                                eps=None if mode == "budget" else s[:, 0] * (0.0617 + 0.003 * np.arange(n_out))))
    return out


def steep(nb, fall=0.6):
    """|rho| and costs falling fast enough that every subset passes the ordering test (the construction of the 26-model case
    of test_gpu_mfmc.py)"""
    k = np.arange(nb + 1)
    return 10.0 ** (-fall * k), np.concatenate([[1.0], 0.9999 ** (k[1:] ** 2)])


def window_cases():
    """nb = 17, complete: 2^17 cliques, more than CAND_CAP of them candidates, so the host loop bisects its windows.  The
    tolerance is loose: the dear models clamp to one sample and only the cheap ones round."""
    w, a = steep(17, 0.3)
    rng = np.random.RandomState(17)
    w = w * rng.uniform(0.97, 1.03, 18)
    out = [case("window_eps_out1", "window", EPS, w, np.ones(18), a, complete(17), eps=0.613),
           case("window_eps_out2", "window", EPS, w, [np.ones(18), rng.uniform(0.8, 1.25, 18)], [a, a ** 1.1], complete(17),
                eps=[0.613, 0.571])]
    return out


def rounding_cases():
    """a winner of 9 models whose model 0 clamps to one sample while the eight cheap ones round: the clamped position has the
    smallest lower bound, so it is bound entry j = 8, and combinations c and c + 256 -- both seen by lane c of k_mfmc_round --
    give the same point.  The first of them must be returned."""
    w, a = steep(9, 0.8)
    w = w * np.random.RandomState(9).uniform(0.97, 1.03, 10)
    return [case("round_eps_nine_models", "round", EPS, w, np.ones(10), a, complete(9), eps=0.0391)]


def ghost(w, s, rho):
    """append a model that changes no sum it enters: |rho| = 3e-12 and a cost of 1.3e-30 w[0].  Its terms (cost m w ~ 1e-25,
    w r ~ 1e-25, variance ~ rho^2 = 1e-23, and rho^2 next to its predecessor's rho^2) vanish in the rounding of every
    accumulation, so a clique and the same clique plus the ghost have bit-identical objectives -- a tie between cliques of
    different sizes, which the size-first rule gives to the smaller one."""
    return (np.concatenate([w, [1.3e-30 * w[0]]]), np.concatenate([s, np.ones((s.shape[0], 1))], axis=1),
            np.concatenate([rho, np.full((rho.shape[0], 1), 3e-12)], axis=1))


def tie_cases():
    """neighbour `dup` is a bit-identical copy (w, s, rho) of neighbour `src`: a clique with one of them ties with the same
    clique with the other (both together fail the ordering test: their rho ratio is x / 0).  The earlier mask, the one
    with `src`, wins.  Placement decides where the two masks meet in the scan: masks below 64 share a wave, below 256 a
    block; above that they differ in block, and for nb >= 21 in grid-stride iteration."""
    out = []
    for label, nb, src, dup, adj in (("same_wave", 5, 3, 4, None), ("same_block", 8, 3, 7, None),
                                     ("other_block", 12, 10, 11, None), ("grid_stride", 21, 19, 20, band(21, 7))):
        n_out = 2
        if nb == 21:
            w, s, rho = wide_inputs(nb, n_out, 5)
        else:
            w, s, rho, _ = hierarchy(nb, n_out, 40 + nb, span=3.0)
        # the copy replaces the last neighbour; the original is the cheapest model before it, so the winner uses one of them
        w[dup + 1], s[:, dup + 1], rho[:, dup + 1] = w[src + 1], s[:, src + 1], rho[:, src + 1]
        for mode in MODES:
            if mode == "small_budget": continue
            out.append(case("tie_%s_%s" % (label, mode), "tie", MODES[mode], w, s, rho, complete(nb) if adj is None else adj,
                            budget=30.79 * w[0] if MODES[mode] & BUDGET else 0.0,
                            eps=None if MODES[mode] & BUDGET else s[:, 0] * np.array([0.127, 0.119]), tie=True, dup=(src, dup)))
    w, s, rho, _ = hierarchy(6, 2, 77, span=3.0)
    w, s, rho = ghost(w, s, rho)
    for mode in ("eps", "budget", "eps_cont", "budget_cont"):
        out.append(case("tie_sizes_%s" % mode, "tie", MODES[mode], w, s, rho, complete(7),
                        budget=30.79 * w[0] if MODES[mode] & BUDGET else 0.0,
                        eps=None if MODES[mode] & BUDGET else s[:, 0] * np.array([0.127, 0.119]), tie=True, ghost=6))
    return out


def small_budget_cases():
    """one nested set of 6 models; the budget steps down so that the full clique pins 0, 1, ..., 5 leading models to one
    sample (5: only the last model is left, with floor(budget / w)); below w[0] nothing is affordable"""
    w = np.array([1.0, 0.9, 0.8, 0.7, 0.6, 0.5]) * np.array([1.0, 1.003, 0.998, 1.004, 0.997, 1.002])
    rho = np.sqrt([1.0, 0.995, 0.989, 0.982, 0.974, 0.965])
    s = np.array([1.0, 1.1, 0.9, 1.2, 0.8, 1.05])
    out = [case("small_budget_%d" % k, "small_budget", SMALL, w, s, rho, complete(5), budget=b)
           for k, b in enumerate((16.418, 14.934, 12.337, 10.853, 10.482, 6.401))]
    out.append(case("small_budget_none", "status", SMALL, w, s, rho, complete(5), budget=0.819))
    return out


def status_cases():
    w, s, rho, _ = hierarchy(3, 1, 5)
    out = [case("none_integer_budget", "status", BUDGET, w, s, rho, complete(3), budget=0.93 * w[0])]
    w, a = steep(25)
    out.append(case("too_big", "status", EPS, w, np.ones(26), a, complete(25), eps=1e-3))
    # |rho_1| = 1 exactly: the lower bound of every clique with neighbour 0 is zero, 2^17 > CAND_CAP of them share it
    w, a = steep(18)
    a[1] = 1.0
    out.append(case("err_state_rho_one", "status", EPS, w, np.ones(19), a, complete(18), eps=0.0913, rc=ref.ERR_STATE,
                    perm=np.arange(19)[None, :]))     # |rho| ties with model 0: it stays first
    return out


def arg_cases():
    """(name, changes to a valid call) -- each must return BLUEST_ERR_ARG before any launch"""
    bad_first = np.array([[1, 0, 2]], dtype=np.int32)
    bad_range = np.array([[0, 1, 3]], dtype=np.int32)
    return [("nb_31", dict(nb=31)), ("n_out_0", dict(n_out=0)), ("n_out_65", dict(n_out=65)),
            ("perm_model0_not_first", dict(perm=bad_first)), ("perm_out_of_range", dict(perm=bad_range)),
            ("eps_mode_without_eps2", dict(eps2=None)), ("null_output", dict(outputs_given=False))]


def valid_small():
    w, s, rho, _ = hierarchy(2, 1, 3)
    return case("valid_small", "base", EPS, w, s, rho, complete(2), eps=0.013 * s[0, 0])


def all_cases():
    return base_cases() + wide_cases() + window_cases() + rounding_cases() + tie_cases() + small_budget_cases() + status_cases()


_RESULTS = {}


def reference(c):
    """the reference's answer for a case, computed once per process and shared"""
    if c["name"] not in _RESULTS:
        _RESULTS[c["name"]] = ref.search(**c["args"])
    return _RESULTS[c["name"]]

"""
Write tests/golden/mlmc_*.npz: setup_mlmc / compute_mlmc_data / attempt_mlmc_setup computed by the REFERENCE (its package and
native module, imported through oracle.gen_golden.import_reference()).  Run where the reference tree exists:

    python tools/gen_golden_mlmc.py

It ends with the reference's setup_mlmc time at n = 12 on one core (kept in profiles/mlmc_cpu_baseline_n12.txt).
"""
import os
import sys
import time
from itertools import combinations

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):     # one BLAS thread for the CPU baseline
    os.environ[_v] = "1"
if hasattr(os, "sched_setaffinity"):
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})          # and one core

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")


def telescoping(n, seed, n_out=1):
    """a telescoping hierarchy: model j = sum_{k >= j} d_k with independent d_k, Var d_k = 4^(-(n-1-k)(1 + 0.25 o)) U(0.8, 1.25)
    for output o, so the difference of two models is small when both are fine.  Costs 2^-j U(0.95, 1.05), model 0 the dearest.
    (A single-factor covariance such as gen_golden_mfmc.chain_cov makes MLMC pick two levels only.)"""
    rng = np.random.RandomState(seed)
    Cs = []
    for o in range(n_out):
        var = 4.0 ** (-(n - 1 - np.arange(n)) * (1 + 0.25 * o)) * rng.uniform(0.8, 1.25, n)
        tail = np.cumsum(var[::-1])[::-1]                                   # Var(model j)
        Cs.append(tail[np.maximum.outer(np.arange(n), np.arange(n))])
    w = 2.0 ** (-np.arange(n)) * rng.uniform(0.95, 1.05, n)
    w[0] = w.max() * 1.01
    return Cs, w


def cases():
    out = []
    for n, seed in ((6, 1), (8, 2), (10, 3)):
        Cs, w = telescoping(n, seed)
        e = 0.01 * np.sqrt(Cs[0][0, 0])
        out.append(("n%d_eps" % n, Cs, w, None, dict(eps=e)))
        out.append(("n%d_budget" % n, Cs, w, None, dict(budget=3000 * w[0])))
        out.append(("n%d_eps_cont" % n, Cs, w, None, dict(eps=e, continuous_relaxation=True)))
        out.append(("n%d_budget_cont" % n, Cs, w, None, dict(budget=3000 * w[0], continuous_relaxation=True)))
    # three outputs; the same problem with an mlmc_variances entry, and with edges cut
    Cs, w = telescoping(7, 5, 3)
    eps3 = [0.01 * np.sqrt(C[0, 0]) * (1 + 0.1 * o) for o, C in enumerate(Cs)]
    out.append(("three_out_eps", Cs, w, None, dict(eps=eps3)))
    out.append(("three_out_budget", Cs, w, None, dict(budget=3000 * w[0])))
    dV = [np.full((7, 7), np.nan) for _ in Cs]
    for n, C in enumerate(Cs): dV[n][1, 3] = 50 * C[1, 1]
    out.append(("three_out_eps_dV", Cs, w, dV, dict(eps=eps3)))
    dVi = [np.full((7, 7), np.nan) for _ in Cs]
    for d in dVi: d[1, 3] = np.inf                                          # not finite: the covariances decide
    out.append(("three_out_eps_dV_inf", Cs, w, dVi, dict(eps=eps3)))
    cut = [C.copy() for C in Cs]
    for C in cut: C[1, 3] = C[3, 1] = np.inf                                # never coupled
    out.append(("three_out_eps_cut13", cut, w, None, dict(eps=eps3)))
    cut = [C.copy() for C in Cs]
    cut[1][0, 1] = cut[1][1, 0] = np.inf                                    # in one output only: the intersection loses the edge
    out.append(("three_out_eps_cut01", cut, w, None, dict(eps=eps3)))
    # unsorted costs: two swapped, one model dearer than model 0 (dropped)
    Cs, w = telescoping(8, 5, 2)
    w = w.copy()
    w[[2, 4]] = w[[4, 2]]
    w[6] = 1.7 * w[0]
    out.append(("unsorted_eps", Cs, w, None, dict(eps=[0.01 * np.sqrt(C[0, 0]) for C in Cs])))
    out.append(("unsorted_budget", Cs, w, None, dict(budget=3000 * w[0])))
    return out


def main():
    from oracle.gen_golden import import_reference
    _, bluest, misc, _ = import_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, Cs, w, dV, kw in cases():
        P = bluest.BLUEProblem(len(w), C=[C.copy() for C in Cs], costs=w, mlmc_variances=dV, n_outputs=len(Cs), verbose=False,
                               skip_projection=True)
        d = P.setup_mlmc(**kw)
        group = [int(g) for g in d["models"]]
        rec = {"C": np.array(Cs), "costs": w, "models": np.array(group), "samples": np.asarray(d["samples"]),
               "errors": np.array(d["errors"]), "total_cost": np.float64(d["total_cost"])}
        if dV is not None: rec["mlmc_variances"] = np.array(dV)
        for k in ("eps", "budget"):
            if k in kw: rec[k] = np.atleast_1d(np.array(kw[k], dtype=np.float64))
        rec["continuous_relaxation"] = np.bool_(kw.get("continuous_relaxation", False))
        cd = P.compute_mlmc_data(group, np.asarray(d["samples"]))
        rec["cd_errors"], rec["cd_total_cost"] = np.array(cd["errors"]), np.float64(cd["total_cost"])
        # the per-output samples on the chosen group
        CC, dd = P.get_covariances(), P.get_mlmc_variances()
        for n in range(len(Cs)):
            sub = CC[n][np.ix_(group, group)]
            subw = w[group].copy()
            if len(group) > 1:
                v = np.diag(sub).copy()
                v[:-1] += v[1:] - 2 * np.diag(sub, 1)
                for i in range(len(group) - 1):
                    check = dd[n][min(group[i], group[i + 1]), max(group[i], group[i + 1])]
                    if np.isfinite(check): v[i] = check
                subw[:-1] += subw[1:]
            else: v = sub[0]
            ok, dn = misc.attempt_mlmc_setup(v, subw, **{k: (val[n] if k == "eps" and np.ndim(val) else val) for k, val in kw.items()})
            rec["out%d_samples" % n] = np.asarray(dn["samples"])
        np.savez(os.path.join(OUT, "mlmc_%s.npz" % name), **rec)
        print(name, group, d["samples"], d["errors"], d["total_cost"])
    # attempt_mlmc_setup on every group of one 5-model problem, in all four modes
    Cs, w = telescoping(5, 6)
    C = Cs[0]
    rec, k = {"C": C, "costs": w}, 0
    modes = (("eps", dict(eps=0.02 * np.sqrt(C[0, 0]))), ("budget", dict(budget=400 * w[0])),
             ("eps_cont", dict(eps=0.02 * np.sqrt(C[0, 0]), continuous_relaxation=True)),
             ("budget_cont", dict(budget=400 * w[0], continuous_relaxation=True)))
    for size in range(1, 6):
        for sub in combinations(range(1, 5), size - 1):
            g = [0] + list(sub)
            subC = C[np.ix_(g, g)]
            subw = w[g].copy()
            if len(g) > 1:
                v = np.diag(subC).copy()
                v[:-1] += v[1:] - 2 * np.diag(subC, 1)
                subw[:-1] += subw[1:]
            else: v = subC[0]
            for mode, kw in modes:
                ok, dd = misc.attempt_mlmc_setup(v, subw, **kw)
                rec["a%d_group" % k], rec["a%d_mode" % k], rec["a%d_ok" % k] = np.array(g), np.array(mode), np.bool_(ok)
                rec["a%d_v" % k], rec["a%d_c" % k] = np.array(v), subw
                if ok:
                    rec["a%d_samples" % k] = np.asarray(dd["samples"])
                    rec["a%d_error" % k], rec["a%d_cost" % k] = np.float64(dd["error"]), np.float64(dd["total_cost"])
                k += 1
    rec["n_attempts"] = np.int64(k)
    for mode, kw in modes: rec["kw_" + mode] = np.float64(kw.get("eps", kw.get("budget")))
    np.savez(os.path.join(OUT, "mlmc_helpers_n5.npz"), **rec)
    # CPU baseline: the reference's setup_mlmc at n = 12 (complete graph, 2^11 groups), one core and one BLAS thread
    Cs, w = telescoping(12, 7)
    P = bluest.BLUEProblem(12, C=[Cs[0].copy()], costs=w, verbose=False, skip_projection=True)
    for kw in (dict(eps=0.01 * np.sqrt(Cs[0][0, 0])), dict(budget=3000 * w[0])):
        ts = []
        for _ in range(3):
            t0 = time.perf_counter()
            d = P.setup_mlmc(**kw)
            ts.append(time.perf_counter() - t0)
        print("reference setup_mlmc n=12 %s: median %.3f s, min %.3f s of 3 (models %s; cores %s)"
              % (list(kw)[0], np.median(ts), min(ts), list(d["models"]), sorted(os.sched_getaffinity(0))))


if __name__ == "__main__":
    main()

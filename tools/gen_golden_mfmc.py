"""
Write tests/golden/mfmc_*.npz: setup_mfmc / compute_mfmc_data / the single-clique helpers of misc.py computed by the REFERENCE
(its package and native module, imported through oracle.gen_golden.import_reference()).  Run where the reference tree exists:

    python tools/gen_golden_mfmc.py
"""
import os
import sys
import time

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):     # one BLAS thread for the CPU baseline
    os.environ[_v] = "1"
if hasattr(os, "sched_setaffinity"):
    os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})          # and one core

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")


def tutorial_cov():
    """tutorials/01_tutorial.py models with the covariance estimated from 2000 samples (seed 0), as tests/test_gpu_api.py does"""
    from scipy.special import gamma
    n = 5

    def series(x, i):
        ii = np.arange(i + 1)
        return np.sum(x ** ii / gamma(ii + 1))
    rng = np.random.RandomState(0)
    Z = rng.randn(2000)
    P = np.array([[np.exp(z)] + [series(z, n - l) for l in range(1, n - 1)] + [np.log(abs(z))] for z in Z])
    return np.cov(P.T), np.array([2.0 ** (n - i) for i in range(n)])


def chain_cov(n, seed, decay=0.08, scale=1.0):
    """X_j = a_j X_0 + noise: |rho_0j| = a_j decreasing with j, costs decreasing geometrically; every pair coupled"""
    rng = np.random.RandomState(seed)
    a = np.concatenate([[1.0], np.sort(1 - decay * np.cumsum(rng.uniform(0.2, 1.0, n - 1)) ** 1.3)[::-1]])
    a = np.clip(a, 0.05, 1.0)
    s = scale * rng.uniform(0.5, 2.0, n)
    R = np.outer(a, a)
    np.fill_diagonal(R, 1.0)
    C = R * np.outer(s, s)
    costs = np.array([float(10 ** (3 - 3.0 * i / (n - 1))) for i in range(n)]) * rng.uniform(0.9, 1.1, n)
    costs[0] = costs.max() * 1.01
    return C, costs


def multi_cov(n, seed, n_out):
    """output o: X_j = a_j^(1 + 0.3 o) X_0 + noise, its own standard deviations; costs as chain_cov"""
    rng = np.random.RandomState(seed)
    a = np.concatenate([[1.0], np.clip(1 - 0.03 * np.cumsum(rng.uniform(0.2, 1.0, n - 1)), 0.05, 1.0)])
    costs = np.array([float(10 ** (3 - 3.0 * i / (n - 1))) for i in range(n)]) * rng.uniform(0.9, 1.1, n)
    costs[0] = costs.max() * 1.01
    Cs = []
    for o in range(n_out):
        ao = a ** (1 + 0.3 * o)
        R = np.outer(ao, ao)
        np.fill_diagonal(R, 1.0)
        s = rng.uniform(0.5, 2.0, n)
        Cs.append(R * np.outer(s, s))
    return Cs, costs


def cases():
    Ct, wt = tutorial_cov()
    out = []
    eps_t = 0.01 * np.sqrt(Ct[0, 0])
    out.append(("tutorial_eps", [Ct], wt, dict(eps=eps_t)))
    out.append(("tutorial_budget", [Ct], wt, dict(budget=100 * wt.max())))
    out.append(("tutorial_small_budget", [Ct], wt, dict(budget=3.3 * wt.max(), small_budget=True)))
    C8, w8 = chain_cov(8, 1)
    out.append(("n8_eps", [C8], w8, dict(eps=0.002 * np.sqrt(C8[0, 0]))))
    out.append(("n8_eps_cont", [C8], w8, dict(eps=0.002 * np.sqrt(C8[0, 0]), continuous_relaxation=True)))
    C10, w10 = chain_cov(10, 2)
    out.append(("n10_budget", [C10], w10, dict(budget=2000 * w10[0])))
    out.append(("n10_budget_cont", [C10], w10, dict(budget=2000 * w10[0], continuous_relaxation=True)))
    C6, w6 = chain_cov(6, 3)
    C6g = C6.copy()
    C6g[2, 4] = C6g[4, 2] = np.inf           # never coupled
    C6g[1, 3] = C6g[3, 1] = 0.0              # uncorrelated
    out.append(("graph_eps", [C6g], w6, dict(eps=0.003 * np.sqrt(C6[0, 0]))))
    out.append(("graph_budget", [C6g], w6, dict(budget=500 * w6[0])))
    C3 = [C6, C6 * 2.5, C6 * np.outer(np.linspace(1, 0.7, 6), np.linspace(1, 0.7, 6))]
    out.append(("three_out_eps", C3, w6, dict(eps=[0.003 * np.sqrt(c[0, 0]) for c in C3])))
    out.append(("three_out_budget", C3, w6, dict(budget=500 * w6[0])))
    # outputs whose correlations differ in value (a_j**(1 + 0.3 o)) but keep one |rho| order: different per-output samples
    Cm, wm = multi_cov(7, 5, 3)
    out.append(("multi_out_eps", Cm, wm, dict(eps=[0.003 * np.sqrt(c[0, 0]) for c in Cm])))
    out.append(("multi_out_budget", Cm, wm, dict(budget=500 * wm[0])))
    R = np.full((4, 4), 0.3) + 0.7 * np.eye(4)
    R[0, 1:] = R[1:, 0] = [0.5, 0.45, 0.4]
    w0 = np.array([1.0, 0.99, 0.98, 0.97])
    out.append(("only_zero", [R], w0, dict(eps=0.05)))
    return out


def main():
    from oracle.gen_golden import import_reference
    _, bluest, misc, _ = import_reference()
    os.makedirs(OUT, exist_ok=True)
    for name, Cs, w, kw in cases():
        P = bluest.BLUEProblem(Cs[0].shape[0], C=Cs, costs=w, n_outputs=len(Cs), verbose=False, skip_projection=True)
        d = P.setup_mfmc(**kw)
        rec = {"C": np.array(Cs), "costs": w, "models": np.array(d["models"]), "samples": np.asarray(d["samples"]),
               "errors": np.array(d["errors"]), "total_cost": np.float64(d["total_cost"]), "alphas": np.concatenate(d["alphas"])}
        for k in ("eps", "budget"):
            if k in kw: rec[k] = np.atleast_1d(np.array(kw[k], dtype=np.float64))
        rec["continuous_relaxation"] = np.bool_(kw.get("continuous_relaxation", False))
        rec["small_budget"] = np.bool_(kw.get("small_budget", False))
        # compute_mfmc_data on the chosen clique with the chosen samples
        cd = P.compute_mfmc_data(list(d["models"]), np.asarray(d["samples"]))
        rec["cd_errors"] = np.array(cd["errors"])
        if len(Cs) > 1:             # the per-output rounded samples on the chosen clique (must differ for the multi_out cases)
            cl = list(d["models"])
            for n, C in enumerate(Cs):
                s = np.sqrt(np.diag(C))
                ok, dn = misc.attempt_mfmc_setup(s[cl], (C / np.outer(s, s))[0][cl], w[cl],
                                                 **{k: (v[n] if k == "eps" else v) for k, v in kw.items()})
                rec["out%d_samples" % n] = np.asarray(dn["samples"])
        rec["cd_total_cost"] = np.float64(cd["total_cost"])
        np.savez(os.path.join(OUT, "mfmc_%s.npz" % name), **rec)
        print(name, d["models"], d["samples"], d["errors"], d["total_cost"])
    # single-clique helpers of misc.py on the tutorial covariance (every clique through model 0)
    Ct, wt = tutorial_cov()
    s = np.sqrt(np.diag(Ct))
    rho = (Ct / np.outer(s, s))[0]
    rec = {"C": Ct, "costs": wt}
    from itertools import combinations
    k = 0
    for size in range(1, 5):
        for sub in combinations(range(1, 5), size - 1):
            cl = [0] + list(sub)
            for mode, kw in (("eps", dict(eps=0.01 * s[0])), ("budget", dict(budget=100 * wt.max())),
                             ("cont", dict(eps=0.01 * s[0], continuous_relaxation=True)),
                             ("low", dict(budget=3.3 * wt.max(), small_budget=True))):
                ok, dd = misc.attempt_mfmc_setup(s[cl], rho[cl], wt[cl], **kw)
                rec["a%d_clique" % k] = np.array(cl)
                rec["a%d_mode" % k] = np.array(mode)
                rec["a%d_ok" % k] = np.bool_(ok)
                if ok:
                    rec["a%d_samples" % k] = np.asarray(dd["samples"])
                    rec["a%d_error" % k] = np.float64(dd["error"])
                    rec["a%d_cost" % k] = np.float64(dd["total_cost"])
                    rec["a%d_alphas" % k] = np.asarray(dd["alphas"])
                k += 1
            m = misc.mfmc_low_budget_integer_solution(rho[cl], wt[cl], 3.3 * wt.max())
            rec["low%d" % (k - 1)] = m
    rec["n_attempts"] = np.int64(k)
    np.savez(os.path.join(OUT, "mfmc_helpers_tutorial.npz"), **rec)
    # CPU baseline: the reference's setup_mfmc at n = 12 (complete graph, 2^11 cliques), one core and one BLAS thread
    # (main() pins both); printed lines are kept in profiles/mfmc_cpu_baseline_n12.txt
    C12, w12 = chain_cov(12, 4)
    P = bluest.BLUEProblem(12, C=C12, costs=w12, verbose=False, skip_projection=True)
    for kw in (dict(eps=0.002 * np.sqrt(C12[0, 0])), dict(budget=2000 * w12[0])):
        P.setup_mfmc(**kw)                                                  # first call: imports and caches
        ts = []
        for _ in range(5):
            t0 = time.perf_counter()
            d = P.setup_mfmc(**kw)
            ts.append(time.perf_counter() - t0)
        print("reference setup_mfmc n=12 %s: median %.3f s, min %.3f s of 5 (models %s; cores %s)"
              % (list(kw)[0], np.median(ts), min(ts), d["models"], sorted(os.sched_getaffinity(0))))

if __name__ == "__main__":
    main()

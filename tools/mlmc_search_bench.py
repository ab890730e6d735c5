"""
Wall time of MLMCMixin.setup_mlmc (the MLMC model-subset search of csrc/mlmc.hip plus its host set-up) on a complete graph:
n = 12 (the shape of the CPU baseline in profiles/mlmc_cpu_baseline_n12.txt) and n = 24 models (nb = 23: 2^23 groups, the
largest of 24 levels, the most the rounding takes, so nothing has to be capped), 1 and 8 outputs, eps and budget mode, integer
rounding.  Needs the GPU; prints one JSON line per shape (kept in profiles/mlmc_search_bench.txt).

    python tools/mlmc_search_bench.py [--sizes 12,24] [--outputs 1,8] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def telescoping(n, seed, n_out=1):
    """the hierarchy of tools/gen_golden_mlmc.py: model j = sum_{k >= j} d_k, Var d_k = 4^(-(n-1-k)(1 + 0.25 o)) U(0.8, 1.25),
    costs 2^-j U(0.95, 1.05), model 0 the dearest"""
    rng = np.random.RandomState(seed)
    Cs = []
    for o in range(n_out):
        var = 4.0 ** (-(n - 1 - np.arange(n)) * (1 + 0.25 * o)) * rng.uniform(0.8, 1.25, n)
        tail = np.cumsum(var[::-1])[::-1]
        Cs.append(tail[np.maximum.outer(np.arange(n), np.arange(n))])
    w = 2.0 ** (-np.arange(n)) * rng.uniform(0.95, 1.05, n)
    w[0] = w.max() * 1.01
    return Cs, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="12,24")
    ap.add_argument("--outputs", default="1,8")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from bluest_amd import BLUEProblem, _lib
    from bluest_amd.mlmc import MLMCMixin

    class Problem(MLMCMixin, BLUEProblem):
        pass
    print(json.dumps({"device": _lib.device_name()}))
    for n in [int(x) for x in args.sizes.split(",")]:
        for n_out in [int(x) for x in args.outputs.split(",")]:
            Cs, w = telescoping(n, 7, n_out)
            P = Problem(n, C=Cs, costs=w, n_outputs=n_out, verbose=False)
            for mode, kw in (("eps", dict(eps=[0.01 * np.sqrt(c[0, 0]) for c in Cs])), ("budget", dict(budget=3000 * w[0]))):
                times = []
                for r in range(args.repeat + 1):                # the first call loads the code object: not timed
                    t0 = time.perf_counter()
                    d = P.setup_mlmc(**kw)
                    if r: times.append(time.perf_counter() - t0)
                print(json.dumps({"n": n, "outputs": n_out, "mode": mode, "groups": 2 ** (n - 1), "models": [int(j) for j in d["models"]],
                                  "median_s": float(np.median(times)), "min_s": float(min(times))}), flush=True)


if __name__ == "__main__":
    main()

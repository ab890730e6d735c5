"""
Wall time of BLUEProblem.setup_mfmc (the MFMC model-subset search of csrc/mfmc.hip plus its host set-up) on a complete graph:
n = 16, 20, 24 models, 1 and 8 outputs, eps and budget mode, integer rounding.  Needs the GPU; prints one JSON line per shape.

    python tools/mfmc_search_bench.py [--sizes 16,20,24] [--outputs 1,8] [--repeat 3]
"""
import argparse
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))


def problem(n, n_out, seed=0):
    """X_j = a_j X_0 + noise with slowly falling a_j and geometric costs: many subsets pass the MFMC ordering condition"""
    rng = np.random.RandomState(seed)
    a = np.concatenate([[1.0], np.clip(1 - 0.02 * np.cumsum(rng.uniform(0.2, 1.0, n - 1)), 0.05, 1.0)])
    w = 10.0 ** (3 - 4.0 * np.arange(n) / (n - 1)) * rng.uniform(0.9, 1.1, n)
    w[0] = w.max() * 1.01
    Cs = []
    for o in range(n_out):
        ao = a ** (1 + 0.05 * o)
        R = np.outer(ao, ao)
        np.fill_diagonal(R, 1.0)
        s = rng.uniform(0.5, 2.0, n)
        Cs.append(R * np.outer(s, s))
    return Cs, w


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default="16,20,24")
    ap.add_argument("--outputs", default="1,8")
    ap.add_argument("--repeat", type=int, default=3)
    args = ap.parse_args()
    from bluest_amd import BLUEProblem, _lib
    print(json.dumps({"device": _lib.device_name()}))
    for n in [int(x) for x in args.sizes.split(",")]:
        for n_out in [int(x) for x in args.outputs.split(",")]:
            Cs, w = problem(n, n_out)
            P = BLUEProblem(n, C=Cs, costs=w, n_outputs=n_out, verbose=False)
            for mode, kw in (("eps", dict(eps=[0.003 * np.sqrt(c[0, 0]) for c in Cs])), ("budget", dict(budget=3000 * w[0]))):
                times = []
                for r in range(args.repeat + 1):                # the first call loads the code object: not timed
                    t0 = time.perf_counter()
                    d = P.setup_mfmc(**kw)
                    if r: times.append(time.perf_counter() - t0)
                print(json.dumps({"n": n, "outputs": n_out, "mode": mode, "cliques": 2 ** (n - 1), "models": [int(j) for j in d["models"]],
                                  "median_s": float(np.median(times)), "min_s": float(min(times))}), flush=True)


if __name__ == "__main__":
    main()

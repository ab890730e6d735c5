"""
Wall time of the SPD covariance projection: BLUEProblem-level bluest_cov_project calls on the GPU, or the reference's
project_covariances on one CPU core with one BLAS thread, on the same matrices (M x M, three slightly negative eigenvalues, 10 %
of the pairs not coupled, so that SPG runs).

    python tools/covproj_bench.py                  # GPU  -> profiles/covproj_bench.txt
    python tools/covproj_bench.py --cpu-reference  # CPU  -> profiles/covproj_cpu_baseline.txt (needs the reference tree)
"""
import os
import sys

CPU = "--cpu-reference" in sys.argv
if CPU:
    for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):
        os.environ[_v] = "1"
    if hasattr(os, "sched_setaffinity"):
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})

import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
SIZES = (12, 20, 40, 64)
OUTPUTS = (1, 8)
REPEAT = 3


def partial_indefinite(M, seed, frac=0.1, neg=0.03):
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(M, M))
    l = rng.uniform(0.2, 2.0, M)
    l[:3] = -neg * rng.uniform(0.5, 1.0, 3)
    C = Q @ np.diag(l) @ Q.T
    C = (C + C.T) / 2
    for i in range(1, M):
        for j in range(i + 1, M):
            if rng.rand() < frac:
                C[i, j] = C[j, i] = np.inf
    return C


def problem(cls, M, n_out):
    Cs = [partial_indefinite(M, 1000 * M + o) for o in range(n_out)]
    costs = np.array([float(10 ** (3 - 3.0 * i / (M - 1))) for i in range(M)])
    return cls(M, C=Cs, costs=costs, n_outputs=n_out, verbose=False, skip_projection=True)


def gpu():
    import torch
    from bluest_amd import _lib, blue_models as bm
    lines = ["# bluest_cov_project on %s: wall time of one project_covariances() (all outputs, one launch), median of %d after "
             "one warm-up; SPG iterations / evaluations per output" % (_lib.device_name(), REPEAT)]
    assert torch.cuda.is_available()
    for M in SIZES:
        for n_out in OUTPUTS:
            p = problem(bm.BLUEProblem, M, n_out)
            Cs = [p.get_covariance(n) for n in range(n_out)]
            args = ([np.where(np.isnan(C), 0.0, C) for C in Cs], [(~np.isnan(C)).astype(np.float64) for C in Cs], bm.spg_default_params)
            res = bm.cov_project(*args)
            ts = []
            for _ in range(REPEAT):
                t0 = time.perf_counter()
                res = bm.cov_project(*args)
                ts.append(time.perf_counter() - t0)
            it = [r[3] for r in res]
            cnt = [r[4] for r in res]
            info = [r[5] for r in res]
            t = float(np.median(ts))
            lines.append("M=%2d n_out=%d  %9.2f ms  %7.1f us per iteration of the slowest output   it %s  count %s  info %s"
                         % (M, n_out, 1e3 * t, 1e6 * t / max(max(it), 1), it, cnt, info))
            print(lines[-1], flush=True)
        # the single clip (every entry known), one output
        C = np.nan_to_num(partial_indefinite(M, 7 * M), posinf=0.0)
        args = ([C], [np.ones((M, M))], bm.spg_default_params)
        bm.cov_project(*args)
        ts = []
        for _ in range(REPEAT):
            t0 = time.perf_counter()
            bm.cov_project(*args)
            ts.append(time.perf_counter() - t0)
        lines.append("M=%2d clip only   %9.2f ms" % (M, 1e3 * float(np.median(ts))))
        print(lines[-1], flush=True)
    return lines, os.path.join(ROOT, "profiles", "covproj_bench.txt")


def cpu():
    import contextlib
    import io
    import platform
    from oracle.gen_golden import import_reference
    _, bluest, _, _ = import_reference()
    import bluest.blue_models as bm
    records = []
    inner = bm.spg

    def spg_rec(*a, **k):
        res = inner(*a, **k)
        records.append((res["it"], res["count"]))
        return res
    bm.spg = spg_rec
    lines = ["# reference BLUEProblem.project_covariances() on one core of %s, one BLAS thread (numpy %s): wall time, median of "
             "%d; SPG iterations / evaluations per output" % (platform.processor() or platform.machine(), np.__version__, REPEAT)]
    for M in SIZES:
        for n_out in OUTPUTS:
            reps = 1 if M >= 40 else REPEAT
            ts = []
            for _ in range(reps):
                p = problem(bluest.BLUEProblem, M, n_out)
                del records[:]
                raised = ""
                t0 = time.perf_counter()
                with contextlib.redirect_stdout(io.StringIO()):
                    try:
                        p.project_covariances()
                    except RuntimeError:             # an output reached maxit: the reference stops there
                        raised = "  RuntimeError after %d of %d outputs" % (len(records), n_out)
                ts.append(time.perf_counter() - t0)
            t = float(np.median(ts))
            its = [r[0] for r in records]
            lines.append("M=%2d n_out=%d  %9.2f ms  %7.1f us per iteration   it %s  count %s%s%s"
                         % (M, n_out, 1e3 * t, 1e6 * t / max(sum(its), 1), its, [r[1] for r in records],
                            "" if reps == REPEAT else "  (one run)", raised))
            print(lines[-1], flush=True)
        C = np.nan_to_num(partial_indefinite(M, 7 * M), posinf=0.0)
        ts = []
        for _ in range(REPEAT):
            t0 = time.perf_counter()
            l, V = np.linalg.eigh(C)
            l[l < 5e-14] = 5e-14
            V @ np.diag(l) @ V.T
            ts.append(time.perf_counter() - t0)
        lines.append("M=%2d clip only   %9.3f ms" % (M, 1e3 * float(np.median(ts))))
        print(lines[-1], flush=True)
    return lines, os.path.join(ROOT, "profiles", "covproj_cpu_baseline.txt")


if __name__ == "__main__":
    lines, path = cpu() if CPU else gpu()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else path
    with open(out, "w") as f:
        f.write("\n".join(lines) + "\n")
    print("wrote", out)

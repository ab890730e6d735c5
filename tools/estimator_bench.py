"""
Wall time of bluest_amd.estimator.group_sums on three shapes, from host and from device memory, against what a user would write
without it:

    python tools/estimator_bench.py [--out FILE]                  # on the GPU machine: group_sums, torch.sum(dim=1) per segment on
                                                                  # the same device tensors, numpy on one core of the same host
    python tools/estimator_bench.py --cpu-reference [--out FILE]  # where the reference tree exists: its blue_fn accumulation on one
                                                                  # core at a small N, SCALED to the shapes' sizes

  large    one segment, 8 outputs x 1 000 000 samples x 3 models (192 MB of float64 values)
  ragged   200 segments of 1..6 models and uneven sample counts, 8 outputs, the same bytes in all
  vartest  50 repeats x 40 groups of 1..3 models, 2 outputs, 10..2000 samples each, with weights: the batch of a variance_test

Both write their own section of FILE (default profiles/estimator_bench.txt) and keep the other one.
"""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):     # one BLAS thread for the CPU figures
    os.environ[_v] = "1"

import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 5
N_REF, BATCH_REF = 2000, 100         # the reference's accumulation is timed at this N, in batches of BATCH_REF
MARK = {"gpu": "## GPU, torch and numpy", "ref": "## reference blue_fn"}


ALL_CORES = os.sched_getaffinity(0) if hasattr(os, "sched_getaffinity") else None


def one_core(on=True):
    if ALL_CORES is not None:
        os.sched_setaffinity(0, {sorted(ALL_CORES)[0]} if on else ALL_CORES)


def cpu_name():
    try:
        for line in open("/proc/cpuinfo"):
            if line.startswith("model name"):
                return line.split(":", 1)[1].strip()
    except OSError:
        pass
    return "unknown CPU"


def median_time(fn, repeat=REPEAT):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def shapes():
    """name -> (n_out, [(N_s, L_s)], repeat_of or None)"""
    rng = np.random.RandomState(5)
    large = [(1000000, 3)]
    widths = rng.randint(1, 7, size=200)
    share = rng.uniform(0.2, 1.8, size=200)
    rows = np.maximum((share / (share * widths).sum() * 3000000).astype(np.int64), 1)      # sum N_s L_s = 3e6 values per output
    ragged = list(zip(rows.tolist(), widths.tolist()))
    groups = list(zip(rng.randint(10, 2001, size=40).tolist(), rng.randint(1, 4, size=40).tolist()))
    return {"large": (8, large, None), "ragged": (8, ragged, None),
            "vartest": (2, groups * 50, np.repeat(np.arange(50), 40))}


def make(n_out, segs, seed=1):
    rng = np.random.RandomState(seed)
    return [1.5 + rng.randn(n_out, N, L) for N, L in segs]


def gpu_section():
    import torch
    from bluest_amd import _lib, estimator
    assert torch.cuda.is_available()
    lines = [MARK["gpu"], "# bluest_group_sums on %s (BLUEST_GSUM_CHUNK = %d); wall time of one synchronous call, median of %d after a "
             "warm-up" % (_lib.device_name(), estimator.BLUEST_GSUM_CHUNK, REPEAT),
             "# torch: [v.sum(dim=1) for v in segments] on the same device tensors, then one synchronise; numpy: the same on one core "
             "of the host (%s)" % cpu_name()]
    for name, (n_out, segs, repeat_of) in shapes().items():
        Y = make(n_out, segs)
        nbytes = sum(v.nbytes for v in Y)
        T = sum(L for _, L in segs)
        W = None if repeat_of is None else np.random.RandomState(2).randn(n_out, T)
        kw = {} if W is None else dict(weights=W, repeat_of=repeat_of)
        host = lambda: estimator.group_sums(Y, slab_bytes=1 << 40, **kw)
        ref = host()
        t_host = median_time(host)
        D = [torch.from_numpy(v).cuda() for v in Y]
        torch.cuda.synchronize()
        dev = lambda: estimator.group_sums(D, **kw)
        got = dev()
        flat = lambda r: np.concatenate((r[0] if W is not None else r), axis=1)
        same = np.array_equal(flat(ref), flat(got)) and (W is None or np.array_equal(ref[1], got[1]))
        t_dev = median_time(dev)

        def torch_sums():
            out = [v.sum(dim=1) for v in D]
            torch.cuda.synchronize()
            return out
        ts = torch_sums()
        close = max(float(np.abs(a.cpu().numpy() - b).max() / np.abs(b).max()) for a, b in zip(ts, (ref[0] if W is not None else ref)))
        t_torch = median_time(torch_sums)

        def torch_host():
            out = [torch.from_numpy(v).cuda().sum(dim=1) for v in Y]
            torch.cuda.synchronize()
            return out
        torch_host()
        t_torch_host = median_time(torch_host)
        one_core()
        t_np = median_time(lambda: [v.sum(axis=1) for v in Y], repeat=3)
        one_core(False)
        lines += ["", "%s: %d segment(s), %d output(s), %d columns, %.1f MB of values%s"
                  % (name, len(segs), n_out, T, nbytes / 1e6, "" if W is None else ", weights and %d repeats" % (repeat_of[-1] + 1)),
                  "  group_sums from device memory   %9.3f ms   (%.0f GB/s of values; same bits as from host memory: %s)"
                  % (t_dev * 1e3, nbytes / t_dev / 1e9, same),
                  "  torch.sum per segment, device   %9.3f ms   (%.2f x group_sums; sums agree to %.1e)" % (t_torch * 1e3, t_torch / t_dev, close),
                  "  group_sums from host memory     %9.3f ms   (pageable; one slab)" % (t_host * 1e3),
                  "  torch: copy + sum per segment   %9.3f ms   (%.2f x group_sums from host memory)" % (t_torch_host * 1e3, t_torch_host / t_host),
                  "  numpy sum(axis=1), one core     %9.3f ms   (%.1f x group_sums from host memory)" % (t_np * 1e3, t_np / t_host)]
        del D
        torch.cuda.empty_cache()
    return lines


def ref_section():
    one_core()
    from oracle.gen_golden import import_reference
    _, bluest, _, _ = import_reference()
    lines = [MARK["ref"], "# the reference's blue_fn with a model that costs nothing, on one core of %s: one group of 3 models, "
             "measured at N = %d" % (cpu_name(), N_REF),
             "# in batches of %d (its fastest form) and SCALED to the shapes above -- not measured at those sizes" % BATCH_REF]
    for name, n_out, scale in (("large", 8, 1000000 / N_REF), ("vartest", 2, 50 * 40 * 1000 / N_REF)):
        Y = 1.5 + np.random.RandomState(1).randn(N_REF // BATCH_REF, n_out, 3, BATCH_REF)

        class Problem(object):
            cost = 1.0

            def __init__(self): self.k = 0

            def evaluate(self, ls, samples):
                self.k += 1
                return [[Y[self.k - 1, n, i] for i in range(3)] for n in range(n_out)]

        def run():
            bluest.blue_fn([0, 1, 2], N_REF, Problem(), sampler=lambda ls, N=1: [0.0] * 3, N1=BATCH_REF, No=n_out, verbose=False)
        t = median_time(run, repeat=3)
        lines += ["%-8s reference blue_fn, %d outputs, N = %d   %9.1f ms   measured;   x %.0f = %9.1f s   scaled to the shape's samples"
                  % (name, n_out, N_REF, t * 1e3, scale, t * scale)]
    return lines


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "estimator_bench.txt")
    which = "ref" if "--cpu-reference" in sys.argv else "gpu"
    sections = {}
    if os.path.exists(out):
        key = None
        for line in open(out).read().splitlines():
            key = next((k for k, m in MARK.items() if line == m), key)
            if key is not None: sections.setdefault(key, []).append(line)
    sections[which] = ref_section() if which == "ref" else gpu_section()
    text = "\n".join("\n".join(sections[k]).rstrip("\n") + "\n" for k in ("gpu", "ref") if k in sections)
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

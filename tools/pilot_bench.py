"""
Wall time of the pilot statistics at N = 100 000 samples, L = 64 models, 8 outputs (410 MB of float64 values):

    python tools/pilot_bench.py [--out FILE]                  # on the GPU machine: bluest_pilot_stats from host and from device
                                                              # memory, the copy's share, and numpy on one core of the same host
    python tools/pilot_bench.py --cpu-reference [--out FILE]  # where the reference tree exists: its blue_fn accumulation on one
                                                              # core, at a smaller N and SCALED to N = 100 000

Both write their own section of FILE (default profiles/pilot_stats_bench.txt) and keep the other one.
"""
import os
import sys

for _v in ("OMP_NUM_THREADS", "OPENBLAS_NUM_THREADS", "MKL_NUM_THREADS"):     # one BLAS thread for the CPU figures
    os.environ[_v] = "1"

import time  # noqa: E402

import numpy as np  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
N, L, N_OUT = 100000, 64, 8
N_REF = 100                          # the reference's accumulation is timed at this N
REPEAT = 3
MARK = {"gpu": "## GPU and numpy", "ref": "## reference blue_fn"}


def one_core():
    if hasattr(os, "sched_setaffinity"):
        os.sched_setaffinity(0, {sorted(os.sched_getaffinity(0))[0]})


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


def numpy_sums(Y):
    """Y.T @ Y plus the explicit differences, per output"""
    out = []
    for y in Y:
        d1, d2 = np.zeros((L, L)), np.zeros((L, L))
        for i in range(L - 1):
            D = y[:, i:i + 1] - y[:, i + 1:]
            d1[i, i + 1:] = D.sum(axis=0)
            d2[i, i + 1:] = np.einsum("si,si->i", D, D)
        out.append((y.sum(axis=0), y.T @ y, d1, d2))
    return out


def gpu_section():
    import torch
    from bluest_amd import _lib, pilot
    assert torch.cuda.is_available()
    Y = 1.5 + np.random.RandomState(1).randn(N_OUT, N, L)
    lines = [MARK["gpu"], "# bluest_pilot_stats on %s, N = %d, L = %d, n_out = %d (%.0f MB of values, BLUEST_PILOT_CHUNK = %d);"
             % (_lib.device_name(), N, L, N_OUT, Y.nbytes / 1e6, pilot.BLUEST_PILOT_CHUNK),
             "# wall time of one call, median of %d after one warm-up" % REPEAT]
    host = lambda: pilot.pilot_statistics(Y, slab_bytes=1 << 40)
    ref = host()
    t_host = median_time(host)
    T = torch.from_numpy(Y).cuda()
    torch.cuda.synchronize()
    dev = lambda: pilot.pilot_statistics(T)
    same = all(np.array_equal(a, b) for a, b in zip(ref, dev()))
    t_dev = median_time(dev)
    nodiff = lambda: pilot.pilot_statistics(T, differences=False)
    nodiff()
    t_nodiff = median_time(nodiff)

    def copy():
        torch.from_numpy(Y).cuda()
        torch.cuda.synchronize()
    copy()
    t_copy = median_time(copy)
    slabs = lambda: pilot.pilot_statistics(Y)
    same_slabs = all(np.allclose(a, b, rtol=1e-12) for a, b in zip(ref, slabs()))
    t_slabs = median_time(slabs)
    lines += ["from host memory (pageable), one call      %9.1f ms" % (t_host * 1e3),
              "from host memory, default (> 256 MB: slabs) %8.1f ms   (output by output; sums agree with the single call: %s)" % (t_slabs * 1e3, same_slabs),
              "from device memory                         %9.1f ms   (same bits as from host memory: %s)" % (t_dev * 1e3, same),
              "from device memory, no difference sums     %9.1f ms" % (t_nodiff * 1e3),
              "host -> device copy of the values alone    %9.1f ms   (%.0f %% of the call from host memory; host minus device: %.1f ms)"
              % (t_copy * 1e3, 100 * t_copy / t_host, (t_host - t_dev) * 1e3)]
    one_core()
    t0 = time.perf_counter()
    mine = numpy_sums(Y)
    t_np = time.perf_counter() - t0
    err = max(float(np.abs(m[3] - r).max() / np.abs(r).max()) for m, r in zip(mine, ref[3]))
    lines += ["# numpy on one core of the same host (%s), one BLAS thread: Y.T @ Y and the explicit differences, one run" % cpu_name(),
              "numpy, one core                            %9.1f ms   (%.0f x the call from host memory, %.0f x from device memory; "
              "sumsd2 agrees to %.1e)" % (t_np * 1e3, t_np / t_host, t_np / t_dev, err)]
    return lines


def ref_section():
    one_core()
    from oracle.gen_golden import import_reference
    _, bluest, _, _ = import_reference()
    Y = 1.5 + np.random.RandomState(1).randn(N_REF, N_OUT, L)

    class Problem(object):
        cost = 1.0

        def __init__(self): self.k = 0

        def evaluate(self, ls, samples):
            self.k += 1
            return [[Y[self.k - 1, n, i] for i in range(L)] for n in range(N_OUT)]

    def run():
        bluest.blue_fn(list(range(L)), N_REF, Problem(), sampler=lambda ls: [0.0] * L, N1=1, No=N_OUT, verbose=False,
                       compute_mlmc_differences=True)
    t = median_time(run)
    return [MARK["ref"], "# the reference's blue_fn(compute_mlmc_differences=True) with a model that costs nothing, on one core of %s:"
            % cpu_name(), "# measured at N = %d (L = %d, n_out = %d, median of %d) and SCALED by %d to N = %d -- not measured at that size"
            % (N_REF, L, N_OUT, REPEAT, N // N_REF, N),
            "reference blue_fn at N = %-6d             %9.1f ms   measured" % (N_REF, t * 1e3),
            "reference blue_fn at N = %-6d             %9.0f s    scaled" % (N, t * N / N_REF)]


def main():
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "pilot_stats_bench.txt")
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

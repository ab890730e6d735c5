"""
Wall time of bluest_amd.moments.group_moments on device-resident values, against bluest_amd.estimator.group_sums on the same bytes
(first moments only: the bandwidth floor this code base reaches) and against what a user would write with torch on the same device:

    python tools/moments_bench.py [--out FILE]          # on the GPU machine; writes profiles/moments_bench.txt

  large    one segment, 8 outputs x 1 000 000 samples x 3 models (192 MB of float64 values)
  ragged   200 segments of 1..6 models and uneven sample counts, 8 outputs, the same bytes in all
  vartest  50 repeats x 40 groups of 1..3 models, 2 outputs, 10..2000 samples each (the shapes of tools/estimator_bench.py)
  wide     one segment, 8 outputs x 100 000 samples x 64 models (410 MB): 2080 pairs per sample
  torch    per segment d = v - v[:, :1], d.sum(dim=1) and einsum('nsi,nsj->nij', d, d), results copied to the host, one synchronise
The library's calls are synchronous and include their allocations and the copy of the results to the host.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 5
FP64_VECTOR_PEAK = 78.6e12          # flop/s, AMD's published FP64 vector figure for the MI355X: half of its FP32 vector rate


def median_time(fn, repeat=REPEAT):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def shapes():
    """name -> (n_out, [(N_s, L_s)]); the first three are those of tools/estimator_bench.py"""
    rng = np.random.RandomState(5)
    widths = rng.randint(1, 7, size=200)
    share = rng.uniform(0.2, 1.8, size=200)
    rows = np.maximum((share / (share * widths).sum() * 3000000).astype(np.int64), 1)      # sum N_s L_s = 3e6 values per output
    groups = list(zip(rng.randint(10, 2001, size=40).tolist(), rng.randint(1, 4, size=40).tolist()))
    return [("large", 8, [(1000000, 3)]), ("ragged", 8, list(zip(rows.tolist(), widths.tolist()))), ("vartest", 2, groups * 50),
            ("wide", 8, [(100000, 64)])]


def main():
    import torch
    from bluest_amd import _lib, estimator, moments
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "moments_bench.txt")
    lines = ["# bluest_group_moments on %s (BLUEST_GSUM_CHUNK = %d); values in device memory, float64; wall time of one synchronous"
             % (_lib.device_name(), estimator.BLUEST_GSUM_CHUNK),
             "# call including its allocations and the copy of the results to the host, median of %d after a warm-up" % REPEAT,
             "# torch: the shifted sums and einsum('nsi,nsj->nij') per segment on the same device tensors, copied to the host "
             "(tools/moments_bench.py)"]
    for name, n_out, segs in shapes():
        torch.manual_seed(len(segs))
        D = [1.5 + torch.randn(n_out, N, L, dtype=torch.float64, device="cuda") for N, L in segs]
        torch.cuda.synchronize()
        nbytes = sum(v.numel() * 8 for v in D)
        ours = lambda: moments.group_moments(D)
        got = ours()
        t_ours = median_time(ours)
        floor = lambda: estimator.group_sums(D)
        floor()
        t_floor = median_time(floor)

        def torch_moments():
            res = []
            for v in D:
                d = v - v[:, :1]
                res.append((d.sum(dim=1).cpu(), torch.einsum("nsi,nsj->nij", d, d).cpu()))
            torch.cuda.synchronize()
            return res
        ref = torch_moments()
        t_torch = median_time(torch_moments, repeat=3)
        agree = max(float(np.abs(s - b.numpy()).max() / max(np.abs(b.numpy()).max(), 1e-300)) for (_, _, s), (_, b) in zip(got, ref))
        fmas = float(sum(n_out * N * L * (L + 1) // 2 for N, L in segs))
        lines += ["", "%s: %d segment(s), %d output(s), %d columns, %d pairs, %.1f MB of values"
                  % (name, len(segs), n_out, sum(L for _, L in segs), sum(L * (L + 1) // 2 for _, L in segs), nbytes / 1e6),
                  "  group_moments                     %9.3f ms   (%.0f GB/s of values; %.2f x group_sums)"
                  % (t_ours * 1e3, nbytes / t_ours / 1e9, t_ours / t_floor),
                  "  group_sums on the same bytes      %9.3f ms   (%.0f GB/s of values)" % (t_floor * 1e3, nbytes / t_floor / 1e9),
                  "  torch shifted einsum per segment  %9.3f ms   (%.2f x group_moments; second moments agree to %.1e)"
                  % (t_torch * 1e3, t_torch / t_ours, agree)]
        if max(L for _, L in segs) == 64:
            lines.append("  fma of the pairs                  %9.3e       (%.2f Tfma/s = %.1f %% of the FP64 vector peak of %.1f TFLOP/s)"
                         % (fmas, fmas / t_ours / 1e12, 100 * 2 * fmas / t_ours / FP64_VECTOR_PEAK, FP64_VECTOR_PEAK / 1e12))
        del D, ref
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

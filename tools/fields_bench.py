"""
Wall time of bluest_amd.fields.field_statistics and field_group_sums on device-resident values, against what a user would write
with torch on the same device:

    python tools/fields_bench.py [--out FILE]          # on the GPU machine; writes profiles/fields_bench.txt

  statistics   (N, L, d) = (100, 8, 100000), (1000, 20, 10000), (10000, 64, 64)
               torch: einsum('sic,c,sjc->ij') for sumsc, sum(dim=0) for sumse, and per model i the explicit differences to the
               models j > i (one [N, L - i - 1, d] tensor at a time) summed for sumsd1 and contracted with w for sumsd2
  sums         one segment of 10000 x 3 x 10000, and 200 ragged segments of the same bytes
               torch: v.sum(dim=0) per segment, then one synchronise
The library's calls return host arrays, torch leaves its results on the device: a second torch figure includes their copy.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 5
STATS = [(100, 8, 100000), (1000, 20, 10000), (10000, 64, 64)]


def median_time(fn, repeat=REPEAT):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def torch_statistics(Y, w, to_host=False):
    import torch
    L = Y.shape[1]
    sumse = Y.sum(dim=0)
    sumsc = torch.einsum("sic,c,sjc->ij", Y, w, Y)
    d1, d2 = [], []
    for i in range(L - 1):
        D = Y[:, i:i + 1] - Y[:, i + 1:]
        d1.append(D.sum(dim=0))
        d2.append(torch.einsum("sjc,c,sjc->j", D, w, D))
    if to_host:
        sumse, sumsc, d1, d2 = sumse.cpu(), sumsc.cpu(), [t.cpu() for t in d1], [t.cpu() for t in d2]
    torch.cuda.synchronize()
    return sumse, sumsc, d1, d2


def stats_section():
    import torch
    from bluest_amd import fields
    lines = []
    for N, L, d in STATS:
        torch.manual_seed(N + L)
        Y = 1.5 + torch.randn(N, L, d, dtype=torch.float64, device="cuda")
        w_host = np.random.RandomState(1).uniform(0.5, 2.0, d)
        w = torch.from_numpy(w_host).cuda()
        torch.cuda.synchronize()
        nbytes = Y.numel() * 8
        ours = lambda: fields.field_statistics(Y, w_host)
        se, sc, d1, d2 = ours()
        t_ours = median_time(ours)
        t_nodiff = median_time(lambda: fields.field_statistics(Y, w_host, differences=False))
        te, tc, t1, t2 = torch_statistics(Y, w)
        t_torch = median_time(lambda: torch_statistics(Y, w))
        t_torch_host = median_time(lambda: torch_statistics(Y, w, to_host=True))
        out_mb = (se.nbytes + sc.nbytes + d2.nbytes + L * (L - 1) // 2 * d * 8) / 1e6
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
        agree = max(rel(se, te.cpu().numpy()), rel(sc, tc.cpu().numpy()),
                    max(rel(d2[i, i + 1:], t2[i].cpu().numpy()) for i in range(L - 1)),
                    max(rel(d1[i, i + 1:], t1[i].cpu().numpy()) for i in range(L - 1)))
        pairs = L * (L + 1) // 2
        flop = 6.0 * N * d * pairs                                      # mul, fma, sub, add, mul, fma per (sample, component, pair)
        lines += ["", "N = %d, L = %d, d = %d: %.1f MB of values, %d pairs, %.1f MB of results copied to the host"
                  % (N, L, d, nbytes / 1e6, pairs, out_mb),
                  "  field_statistics                  %9.3f ms   (%.0f GB/s of values, %.2f TFLOP/s of its %.0f flop/B)"
                  % (t_ours * 1e3, nbytes / t_ours / 1e9, flop / t_ours / 1e12, flop / nbytes),
                  "  field_statistics, no differences  %9.3f ms" % (t_nodiff * 1e3),
                  "  torch einsum + differences        %9.3f ms   (%.2f x field_statistics; results agree to %.1e)"
                  % (t_torch * 1e3, t_torch / t_ours, agree),
                  "  torch, results copied to the host %9.3f ms" % (t_torch_host * 1e3)]
        del Y
        torch.cuda.empty_cache()
    return lines


def sums_section():
    import torch
    from bluest_amd import fields
    rng = np.random.RandomState(5)
    widths = rng.randint(1, 7, size=200)
    d = 10000
    share = rng.uniform(0.2, 1.8, size=200)
    rows = np.maximum((share / (share * widths).sum() * 30000).astype(np.int64), 1)        # sum N_s L_s = 3e4 rows of d values
    lines = []
    for name, segs in (("one segment", [(10000, 3)]), ("ragged", list(zip(rows.tolist(), widths.tolist())))):
        torch.manual_seed(len(segs))
        D = [1.5 + torch.randn(N, L, d, dtype=torch.float64, device="cuda") for N, L in segs]
        torch.cuda.synchronize()
        nbytes = sum(v.numel() * 8 for v in D)
        ours = lambda: fields.field_group_sums(D)
        got = ours()
        t_ours = median_time(ours)

        def torch_sums(to_host=False):
            out = [v.sum(dim=0) for v in D]
            if to_host:
                out = [t.cpu() for t in out]
            torch.cuda.synchronize()
            return out
        ts = torch_sums()
        t_torch = median_time(torch_sums)
        t_torch_host = median_time(lambda: torch_sums(True))
        out_mb = sum(v.nbytes for v in got) / 1e6
        agree = max(float(np.abs(a.cpu().numpy() - b).max() / np.abs(b).max()) for a, b in zip(ts, got))
        lines += ["", "%s: %d segment(s) of d = %d, %d columns, %.1f MB of values, %.1f MB of results copied to the host"
                  % (name, len(segs), d, sum(L for _, L in segs), nbytes / 1e6, out_mb),
                  "  field_group_sums                  %9.3f ms   (%.0f GB/s of values)" % (t_ours * 1e3, nbytes / t_ours / 1e9),
                  "  torch.sum(dim=0) per segment      %9.3f ms   (%.2f x field_group_sums, %.0f GB/s; sums agree to %.1e)"
                  % (t_torch * 1e3, t_torch / t_ours, nbytes / t_torch / 1e9, agree),
                  "  torch, results copied to the host %9.3f ms" % (t_torch_host * 1e3)]
        del D
        torch.cuda.empty_cache()
    return lines


def main():
    import torch
    from bluest_amd import _lib, fields
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "fields_bench.txt")
    lines = ["# bluest_field_stats / bluest_field_sums on %s (BLUEST_FIELD_TILE = %d); values in device memory, float64; wall time of one"
             % (_lib.device_name(), fields.BLUEST_FIELD_TILE),
             "# synchronous call including its allocations and the copy of the results to the host, median of %d after a warm-up" % REPEAT,
             "# torch: the same quantities with torch on the same device tensors, then one synchronise (tools/fields_bench.py)",
             "", "## statistics"] + stats_section() + ["", "## sums"] + sums_section()
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

"""
Wall time of bluest_amd.field_errors.field_weighted_moments on device-resident values, against field_group_sums on the same
segments -- it reads the same bytes once, so it is the yardstick -- and against what a user would write with torch:

    python tools/field_errors_bench.py [--out FILE]    # on the GPU machine; writes profiles/field_errors_bench.txt

  shapes   (N, L, d) = (100, 8, 100000), (1000, 20, 10000), (10000, 64, 64) and one segment of 10000 x 3 x 10000: those of
           tools/fields_bench.py
  torch    z = ((v - v[:1]) * coef[None, :, None]).sum(1), then z.sum(0) and (z * z).sum(0), then one synchronise
The two library calls are timed alternately, one after the other, REPEAT times.  They return host arrays, torch leaves its results
on the device: a second torch figure includes their copy.  No ratio is fixed in advance; the file records what was measured.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 9
SHAPES = [(100, 8, 100000), (1000, 20, 10000), (10000, 64, 64), (10000, 3, 10000)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    import torch
    from bluest_amd import _lib, field_errors, fields
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "field_errors_bench.txt")
    lines = ["# bluest_field_weighted_moments on %s (BLUEST_GSUM_CHUNK = 128); values in device memory, float64; wall time of one"
             % _lib.device_name(),
             "# synchronous call including its allocations and the copy of the results to the host; median (and range) of %d after a" % REPEAT,
             "# warm-up, field_weighted_moments and field_group_sums alternating; torch: the same quantities with torch on the same",
             "# device tensor, then one synchronise (tools/field_errors_bench.py)"]
    for N, L, d in SHAPES:
        torch.manual_seed(N + L)
        v = 1.5 + torch.randn(N, L, d, dtype=torch.float64, device="cuda")
        coef_host = np.random.RandomState(L).randn(L)
        coef = torch.from_numpy(coef_host).cuda()
        torch.cuda.synchronize()
        nbytes = v.numel() * 8
        ours = lambda: field_errors.field_weighted_moments([v], coef_host)
        sums = lambda: fields.field_group_sums([v])

        def torch_moments(to_host=False):
            z = ((v - v[:1]) * coef[None, :, None]).sum(1)
            a, b = z.sum(0), (z * z).sum(0)
            if to_host:
                a, b = a.cpu(), b.cpu()
            torch.cuda.synchronize()
            return a, b
        (_, zsum, zsq), = ours()
        sums()
        ta, tb = torch_moments()
        t_ours, t_sums = [], []
        for _ in range(REPEAT):
            t_ours.append(timed(ours))
            t_sums.append(timed(sums))
        t_torch = [timed(torch_moments) for _ in range(REPEAT)]
        t_torch_host = [timed(lambda: torch_moments(True)) for _ in range(REPEAT)]
        m_ours, m_sums, m_torch = float(np.median(t_ours)), float(np.median(t_sums)), float(np.median(t_torch))
        rel = lambda a, b: float(np.abs(a - b).max() / np.abs(b).max())
        agree = max(rel(zsum, ta.cpu().numpy()), rel(zsq, tb.cpu().numpy()))
        lines += ["", "N = %d, L = %d, d = %d: %.1f MB of values; %.2f MB of results copied to the host by field_weighted_moments, %.2f MB by field_group_sums"
                  % (N, L, d, nbytes / 1e6, 2 * d * 8 / 1e6, L * d * 8 / 1e6),
                  "  field_weighted_moments            %9.3f ms   (%.3f .. %.3f; %.0f GB/s of values)"
                  % (m_ours * 1e3, min(t_ours) * 1e3, max(t_ours) * 1e3, nbytes / m_ours / 1e9),
                  "  field_group_sums                  %9.3f ms   (%.3f .. %.3f; %.0f GB/s of values; %.2f x field_weighted_moments)"
                  % (m_sums * 1e3, min(t_sums) * 1e3, max(t_sums) * 1e3, nbytes / m_sums / 1e9, m_sums / m_ours),
                  "  torch expression                  %9.3f ms   (%.2f x field_weighted_moments; results agree to %.1e)"
                  % (m_torch * 1e3, m_torch / m_ours, agree),
                  "  torch, results copied to the host %9.3f ms" % (float(np.median(t_torch_host)) * 1e3)]
        del v
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

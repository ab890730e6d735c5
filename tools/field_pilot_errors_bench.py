"""
Wall time of bluest_amd.field_pilot_errors.field_pilot_moments on device-resident values, against fields.field_statistics with
difference sums on the same tensor -- the same two fmas per (pair, sample, component), the yardstick -- and against what a user
would write with torch:

    python tools/field_pilot_errors_bench.py [--out FILE]    # on the GPU machine; writes profiles/field_pilot_errors_bench.txt

  shapes   (N, L, d) = (100, 8, 100000), (1000, 20, 10000), (10000, 64, 64) and 10000 x 3 x 10000: those of tools/fields_bench.py
  centre   the per-component mean, formed once before the clock starts (the mix-in has it from the sums of field_statistics)
  torch    X = v - centre; q = einsum('sic,c,sjc->sij', X, w, X); q.sum(0), (q * q).sum(0), then one synchronise (no differences)
The two library calls are timed alternately, one after the other, REPEAT times after a warm-up.  They return host arrays; torch
leaves its results on the device.  No ratio is fixed in advance; the file records what was measured.  The kernel times come from
a run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/field_pilot_errors_bench.py --out /dev/null
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 9
SHAPES = [(100, 8, 100000), (1000, 20, 10000), (10000, 64, 64), (10000, 3, 10000)]
STRIP = 512


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(ts):
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    import torch
    from bluest_amd import _lib, field_pilot_errors, fields
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "field_pilot_errors_bench.txt")
    lines = ["# bluest_field_pilot_moments on %s (BLUEST_PILOT_CHUNK = 128, BLUEST_FIELD_STRIP = 512); values in device memory, float64;" % _lib.device_name(),
             "# wall time of one synchronous call including its allocations and the copy of the results to the host; median (and range)",
             "# of %d after a warm-up, field_pilot_moments and field_statistics (both with the difference sums) alternating; torch: the" % REPEAT,
             "# per-sample inner products of the centred values and their two sums on the same device tensor, without the differences,",
             "# then one synchronise (tools/field_pilot_errors_bench.py).  Clocks: as the machine had them, not pinned."]

    def torch_moments(v, w, centre):
        X = v - centre
        q = torch.einsum("sic,c,sjc->sij", X, w, X)
        res = (q.sum(0), (q * q).sum(0))
        torch.cuda.synchronize()
        return q, res

    for N, L, d in SHAPES:
        torch.manual_seed(N + L)
        v = 1.5 + torch.randn(N, L, d, dtype=torch.float64, device="cuda")
        w_host = np.random.RandomState(L).uniform(0.5, 2.0, d)
        w = torch.from_numpy(w_host).cuda()
        centre_host = fields.field_statistics(v, w_host, differences=False)[0] / N
        centre = torch.from_numpy(centre_host).cuda()
        torch.cuda.synchronize()
        nbytes = v.numel() * 8
        nstrips = (d - 1) // STRIP + 1
        scratch = N * (nstrips + (nstrips > 1)) * L * (L + 1) * 8
        ours = lambda: field_pilot_errors.field_pilot_moments(v, w_host, centre_host)
        stats = lambda: fields.field_statistics(v, w_host, differences=True)
        got = ours()
        stats()
        q, _ = torch_moments(v, w, centre)
        mean = (got[0] + got[1] / N)
        agree = float(np.abs(mean - q.mean(0).cpu().numpy()).max() / np.abs(mean).max())
        del q
        t_ours, t_stats = [], []
        for _ in range(REPEAT):
            t_ours.append(timed(ours))
            t_stats.append(timed(stats))
        t_q = [timed(lambda: field_pilot_errors.field_pilot_moments(v, w_host, centre_host, differences=False)) for _ in range(REPEAT)]
        t_torch = [timed(lambda: torch_moments(v, w, centre)) for _ in range(REPEAT)]
        m_ours, m_stats, m_torch = summary(t_ours), summary(t_stats), summary(t_torch)
        lines += ["", "N = %d, L = %d, d = %d: %.1f MB of values; per-sample scratch %.1f MB (%.1f %% of the values); %.4f MB of results copied to the host, %.2f MB by field_statistics"
                  % (N, L, d, nbytes / 1e6, scratch / 1e6, 100.0 * scratch / nbytes, 6 * L * L * 8 / 1e6, (L * d + 2 * L * L + L * (L - 1) // 2 * d) * 8 / 1e6),
                  "  field_pilot_moments               %9.3f ms   (%.3f .. %.3f; %.0f GB/s of values)" % (m_ours + (nbytes / m_ours[0] / 1e6,)),
                  "  field_pilot_moments, q only       %9.3f ms" % summary(t_q)[0],
                  "  field_statistics, differences     %9.3f ms   (%.3f .. %.3f; field_pilot_moments takes %.2f x this)"
                  % (m_stats + (m_ours[0] / m_stats[0],)),
                  "  torch expression, q only          %9.3f ms   (%.2f x field_pilot_moments, q only; the means of q agree to %.1e)"
                  % (m_torch[0], m_torch[0] / summary(t_q)[0], agree)]
        del v
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

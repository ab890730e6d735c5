"""
Wall time of one segment streamed through bluest_amd.field_stream.FieldAccumulator in device batches, against the two one-shot
calls -- field_group_sums and field_weighted_moments -- on the same tensor held whole:

    python tools/field_stream_bench.py [--out FILE]    # on the GPU machine; writes profiles/field_stream_bench.txt

  shapes    (N, L, d) = (10000, 3, 10000) and (10000, 64, 64)
  streamed  one accumulator with coefficients, updates of BATCH = 500 rows (views of the same device tensor: nothing is copied
            but the rows that straddle a chunk), finish; every update synchronises
  held      field_group_sums([v]) and field_weighted_moments([v], coef), one after the other
Both return their results on the host, and both give the same bits (asserted).  Median and range of REPEAT after a warm-up, the
two timed alternately.  No ratio is fixed in advance; the file records what was measured.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 9
BATCH = 500
SHAPES = [(10000, 3, 10000), (10000, 64, 64)]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def main():
    import torch
    from bluest_amd import _lib, field_errors, field_stream, fields
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "field_stream_bench.txt")
    lines = ["# one segment streamed through bluest_field_accum_* in device batches of %d rows on %s, against bluest_field_sums +"
             % (BATCH, _lib.device_name()),
             "# bluest_field_weighted_moments on the same tensor held whole; float64, values in device memory, results copied to the",
             "# host, the same bits both ways; wall time, median (and range) of %d after a warm-up, the two alternating" % REPEAT,
             "# (tools/field_stream_bench.py)"]
    for N, L, d in SHAPES:
        torch.manual_seed(N + L)
        v = 1.5 + torch.randn(N, L, d, dtype=torch.float64, device="cuda")
        coef = np.random.RandomState(L).randn(L)
        torch.cuda.synchronize()
        nbytes = v.numel() * 8
        info = []

        def streamed():
            with field_stream.FieldAccumulator(L, d, coef) as acc:
                for lo in range(0, N, BATCH):
                    acc.update(v[lo:lo + BATCH])
                del info[:]
                info.extend(acc.info())
                return acc.finish()

        def held():
            return fields.field_group_sums([v])[0], field_errors.field_weighted_moments([v], coef)[0]
        got, (sums, (_, zsum, zsq)) = streamed(), held()
        same = lambda a, b: np.array_equal(a.view(np.int64), b.view(np.int64))
        assert got[0] == N and same(got[1], sums) and same(got[2], zsum) and same(got[3], zsq)
        t_s, t_h = [], []
        for _ in range(REPEAT):
            t_s.append(timed(streamed))
            t_h.append(timed(held))
        m_s, m_h = float(np.median(t_s)), float(np.median(t_h))
        updates = -(-N // BATCH)
        # the carry reads a partial and reads and writes a lane per chunk and column: 3 (W + 2 d) doubles against the chunk's 128 W
        carry = 3.0 * (L * d + 2 * d) / (128.0 * L * d)
        lines += ["", "N = %d, L = %d, d = %d: %.1f MB of values in %d updates of %d rows (%.1f MB each, %.1f chunks)"
                  % (N, L, d, nbytes / 1e6, updates, BATCH, BATCH * L * d * 8 / 1e6, BATCH / 128.0),
                  "  held whole: field_group_sums + field_weighted_moments   %9.3f ms   (%.3f .. %.3f; the values are read twice: %.0f GB/s)"
                  % (m_h * 1e3, min(t_h) * 1e3, max(t_h) * 1e3, 2 * nbytes / m_h / 1e9),
                  "  streamed: create, %3d updates, finish                   %9.3f ms   (%.3f .. %.3f; %.0f GB/s; %.2f x held whole)"
                  % (updates, m_s * 1e3, min(t_s) * 1e3, max(t_s) * 1e3, 2 * nbytes / m_s / 1e9, m_s / m_h),
                  "  per update %.3f ms; the carry's bytes are %.1f %% of the values' (computed, not measured); device state held %.1f MB; "
                  "%d device allocations over the run" % (m_s / updates * 1e3, 100 * carry, info[6] / 1e6, info[3])]
        del v
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

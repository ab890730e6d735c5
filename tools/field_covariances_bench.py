"""
Wall time of bluest_amd.field_covariances.field_group_moments on device-resident values, against fields.field_statistics without
difference sums on the same tensor -- parent code with the same number of fmas per pair, the yardstick -- and against what a user
would write with torch:

    python tools/field_covariances_bench.py [--out FILE]    # on the GPU machine; writes profiles/field_covariances_bench.txt

  shapes   (N, L, d) = (100, 8, 100000), (1000, 20, 10000), (10000, 64, 64) and one segment of 10000 x 3 x 10000: those of
           tools/fields_bench.py; then 200 ragged segments of 50 samples, L = 1..5 in turn, d = 10000: the bytes of the last shape
           (field_statistics takes one array: the ragged call has only the torch expression, segment by segment, beside it)
  torch    D = v - v[:1]; einsum('ijc,c,ikc->jk', D, w, D), f = D.sum(0), einsum('jc,c,kc->jk', f, w, f), then one synchronise
The two library calls are timed alternately, one after the other, REPEAT times after a warm-up.  They return host arrays, torch
leaves its results on the device: a second torch figure includes their copy.  No ratio is fixed in advance; the file records what
was measured.  The kernel times come from a run of their own:
    rocprofv3 --kernel-trace --stats -d DIR -- python tools/field_covariances_bench.py --out /dev/null
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 9
SHAPES = [(100, 8, 100000), (1000, 20, 10000), (10000, 64, 64), (10000, 3, 10000)]
RAGGED = (200, 50, 10000)                                               # segments, samples of each, components


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(ts):
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    import torch
    from bluest_amd import _lib, field_covariances, fields
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "field_covariances_bench.txt")
    lines = ["# bluest_field_group_moments on %s (BLUEST_GSUM_CHUNK = 128, BLUEST_FIELD_TILE = 8); values in device memory, float64;" % _lib.device_name(),
             "# wall time of one synchronous call including its allocations and the copy of the results to the host; median (and range)",
             "# of %d after a warm-up, field_group_moments and field_statistics alternating; torch: the same quantities with torch on the" % REPEAT,
             "# same device tensor, then one synchronise (tools/field_covariances_bench.py).  Clocks: as the machine had them, not pinned."]

    def torch_moments(vs, w, to_host=False):
        res = []
        for v in vs:
            D = v - v[:1]
            f = D.sum(0)
            res.append((torch.einsum("ijc,c,ikc->jk", D, w, D), torch.einsum("jc,c,kc->jk", f, w, f)))
        if to_host:
            res = [(a.cpu(), b.cpu()) for a, b in res]
        torch.cuda.synchronize()
        return res

    def agreement(got, want):
        worst = 0.0
        for (N, second, cross), (a, b) in zip(got, want):
            a, b = a.cpu().numpy(), b.cpu().numpy()
            worst = max(worst, float(np.abs(second - a).max() / np.abs(a).max()), float(np.abs(cross - b).max() / max(np.abs(b).max(), 1e-300)))
        return worst

    for N, L, d in SHAPES:
        torch.manual_seed(N + L)
        v = 1.5 + torch.randn(N, L, d, dtype=torch.float64, device="cuda")
        w_host = np.random.RandomState(L).uniform(0.5, 2.0, d)
        w = torch.from_numpy(w_host).cuda()
        torch.cuda.synchronize()
        nbytes = v.numel() * 8
        ours = lambda: field_covariances.field_group_moments([v], w_host)
        stats = lambda: fields.field_statistics(v, w_host, differences=False)
        got = ours()
        stats()
        agree = agreement(got, torch_moments([v], w))
        t_ours, t_stats = [], []
        for _ in range(REPEAT):
            t_ours.append(timed(ours))
            t_stats.append(timed(stats))
        t_first = [timed(lambda: field_covariances.field_group_moments([v], w_host, with_first=True)) for _ in range(REPEAT)]
        t_torch = [timed(lambda: torch_moments([v], w)) for _ in range(REPEAT)]
        t_torch_host = [timed(lambda: torch_moments([v], w, True)) for _ in range(REPEAT)]
        m_ours, m_stats, m_torch = summary(t_ours), summary(t_stats), summary(t_torch)
        lines += ["", "N = %d, L = %d, d = %d: %.1f MB of values; %.4f MB of results copied to the host by field_group_moments, %.2f MB by field_statistics"
                  % (N, L, d, nbytes / 1e6, L * (L + 1) * 8 / 1e6, (L * d + L * L) * 8 / 1e6),
                  "  field_group_moments               %9.3f ms   (%.3f .. %.3f; %.0f GB/s of values)" % (m_ours + (nbytes / m_ours[0] / 1e6,)),
                  "  field_group_moments, with first   %9.3f ms" % summary(t_first)[0],
                  "  field_statistics, no differences  %9.3f ms   (%.3f .. %.3f; %.0f GB/s of values; %.2f x field_group_moments)"
                  % (m_stats + (nbytes / m_stats[0] / 1e6, m_stats[0] / m_ours[0])),
                  "  torch expression                  %9.3f ms   (%.2f x field_group_moments; results agree to %.1e)" % (m_torch[0], m_torch[0] / m_ours[0], agree),
                  "  torch, results copied to the host %9.3f ms" % summary(t_torch_host)[0]]
        del v
        torch.cuda.empty_cache()

    S, N, d = RAGGED
    torch.manual_seed(S)
    vs = [1.5 + torch.randn(N, 1 + s % 5, d, dtype=torch.float64, device="cuda") for s in range(S)]
    w_host = np.random.RandomState(S).uniform(0.5, 2.0, d)
    w = torch.from_numpy(w_host).cuda()
    torch.cuda.synchronize()
    nbytes = sum(v.numel() for v in vs) * 8
    ours = lambda: field_covariances.field_group_moments(vs, w_host)
    agree = agreement(ours(), torch_moments(vs, w))
    t_ours = [timed(ours) for _ in range(REPEAT)]
    t_first = [timed(lambda: field_covariances.field_group_moments(vs, w_host, with_first=True)) for _ in range(REPEAT)]
    t_sums = [timed(lambda: fields.field_group_sums(vs)) for _ in range(REPEAT)]
    t_torch = [timed(lambda: torch_moments(vs, w)) for _ in range(REPEAT)]
    m_ours, m_torch = summary(t_ours), summary(t_torch)
    lines += ["", "%d ragged segments of %d samples, L = 1..5 in turn, d = %d: %.1f MB of values" % (S, N, d, nbytes / 1e6),
              "  field_group_moments               %9.3f ms   (%.3f .. %.3f; %.0f GB/s of values)" % (m_ours + (nbytes / m_ours[0] / 1e6,)),
              "  field_group_moments, with first   %9.3f ms   (%.1f MB more to the host)" % (summary(t_first)[0], sum(v.shape[1] for v in vs) * d * 8 / 1e6),
              "  field_group_sums                  %9.3f ms   (the same bytes read once, the per-component sums copied to the host)" % summary(t_sums)[0],
              "  torch expression, per segment     %9.3f ms   (%.2f x field_group_moments; results agree to %.1e)" % (m_torch[0], m_torch[0] / m_ours[0], agree)]
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

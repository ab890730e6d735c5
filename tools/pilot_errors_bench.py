"""
Wall time of bluest_amd.pilot_errors.pilot_fourth_moments on device-resident values, against bluest_amd.pilot.pilot_statistics on
the same tensor (the yardstick: the same LDS reads with a third to a half of the arithmetic per pair and sample) and against what
a user would write with torch.einsum on the same device:

    python tools/pilot_errors_bench.py [--out FILE]     # on the GPU machine; writes profiles/pilot_errors_bench.txt

  shapes   (N, L, n_out) = (100 000, 64, 8), (100 000, 8, 8), (10 000, 64, 1)
  call     one synchronous call including its allocations and the copy of the results to the host, median of REPEAT after a warm-up
  kernels  the durations of the call's kernels alone, from `rocprofv3 --kernel-trace` over a child process that makes the same calls
           (a run of its own: tracing slows the host, so the wall times above are taken without it)
  torch    d = v - v[:, :1]; d.sum(1), einsum('nsi,nsj->nij') of (d, d), (d^2, d), (d^2, d^2), and per output the explicit differences
           t and the sums of t, t^2, t^3, t^4; results copied to the host, one synchronise
"""
import csv
import glob
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 5
SHAPES = [(100000, 64, 8), (100000, 8, 8), (10000, 64, 1)]
FP64_VECTOR_PEAK = 78.6e12          # flop/s, AMD's published FP64 vector figure for the MI355X (an fma counts two)
# the kernels of one call of either entry point, in launch order
KERNELS = (("k_p4_partial", "k_p4_fold"), ("k_pilot_partial", "k_pilot_fold"))


def median_time(fn, repeat=REPEAT):
    ts = []
    for _ in range(repeat):
        t0 = time.perf_counter()
        fn()
        ts.append(time.perf_counter() - t0)
    return float(np.median(ts))


def values(N, L, n_out):
    import torch
    torch.manual_seed(N + L + n_out)
    v = 1.5 + torch.randn(n_out, N, L, dtype=torch.float64, device="cuda")
    torch.cuda.synchronize()
    return v


def torch_moments(v):
    import torch
    d = v - v[:, :1]
    d2 = d * d
    res = [d.sum(dim=1).cpu(), torch.einsum("nsi,nsj->nij", d, d).cpu(), torch.einsum("nsi,nsj->nij", d2, d).cpu(),
           torch.einsum("nsi,nsj->nij", d2, d2).cpu()]
    tp = []
    for y in v:                                                         # output by output: N x L x L doubles at a time
        a = y[0]
        t = (y[:, :, None] - y[:, None, :]) - (a[:, None] - a[None, :])
        t2 = t * t
        tp.append(torch.stack([t.sum(dim=0), t2.sum(dim=0), (t2 * t).sum(dim=0), (t2 * t2).sum(dim=0)]).triu(1).cpu())
    res.append(torch.stack(tp))
    torch.cuda.synchronize()
    return res


def trace_child():
    """the calls alone, for the kernel trace: per shape 1 + REPEAT calls of each entry point"""
    from bluest_amd import pilot, pilot_errors
    for N, L, n_out in SHAPES:
        v = values(N, L, n_out)
        for _ in range(1 + REPEAT):
            pilot_errors.pilot_fourth_moments(v)
        for _ in range(1 + REPEAT):
            pilot.pilot_statistics(v)
        del v


def kernel_times():
    """per shape ({kernel: median us over the REPEAT timed calls}) from a traced child process, in SHAPES order"""
    with tempfile.TemporaryDirectory() as tmp:
        cmd = ["rocprofv3", "--kernel-trace", "--output-format", "csv", "-d", tmp, "-o", "trace", "--", sys.executable,
               os.path.abspath(__file__), "--trace-child"]
        subprocess.run(cmd, check=True, timeout=300, stdout=subprocess.DEVNULL, stderr=subprocess.PIPE)
        files = glob.glob(os.path.join(tmp, "**", "*kernel_trace.csv"), recursive=True)
        if len(files) != 1:
            raise RuntimeError("expected one kernel trace, found %s" % files)
        rows = sorted((int(r["Start_Timestamp"]), int(r["End_Timestamp"]), r["Kernel_Name"]) for r in csv.DictReader(open(files[0])))
    ours = [(n, (e - s) / 1e3) for s, e, n in rows if "k_p4_" in n or "k_pilot_" in n]
    out = []
    for _ in SHAPES:
        shape = {}
        for labels in KERNELS:
            n = len(labels) * (1 + REPEAT)
            block, ours = ours[:n], ours[n:]
            if len(block) != n or not all(labels[j % len(labels)].split(" ")[0] in name for j, (name, _) in enumerate(block)):
                raise RuntimeError("the trace does not hold the calls in the order they were made")
            timed = block[len(labels):]                                 # without the warm-up call
            for j, label in enumerate(labels):
                shape[label] = float(np.median([us for _, us in timed[j::len(labels)]]))
        out.append(shape)
    return out


def main():
    import torch
    from bluest_amd import _lib, pilot, pilot_errors
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "pilot_errors_bench.txt")
    lines = ["# bluest_pilot_moments4 on %s (BLUEST_PILOT_CHUNK = %d); values in device memory, float64; wall time of one synchronous"
             % (_lib.device_name(), pilot.BLUEST_PILOT_CHUNK),
             "# call including its allocations and the copy of the results to the host, median of %d after a warm-up; kernels: durations"
             % REPEAT,
             "# from rocprofv3 --kernel-trace over a child process making the same calls, median of %d dispatches; torch: the same sums"
             % REPEAT,
             "# with einsum and explicit differences on the same tensor, copied to the host (tools/pilot_errors_bench.py)"]
    calls = []
    for N, L, n_out in SHAPES:
        v = values(N, L, n_out)
        ours = lambda: pilot_errors.pilot_fourth_moments(v)
        got = ours()
        t_ours = median_time(ours)
        nodiff = lambda: pilot_errors.pilot_fourth_moments(v, differences=False)
        nodiff()
        t_nodiff = median_time(nodiff)
        yard = lambda: pilot.pilot_statistics(v)
        yard()
        t_yard = median_time(yard)
        ref = torch_moments(v)
        t_torch = median_time(lambda: torch_moments(v), repeat=3)
        agree = max(float(np.abs(g - r.numpy()).max() / max(np.abs(r.numpy()).max(), 1e-300)) for g, r in zip(got[1:], ref))
        calls.append((t_ours, t_nodiff, t_yard, t_torch, agree))
        del v, ref
        torch.cuda.empty_cache()
    traced = kernel_times()
    for (N, L, n_out), (t_ours, t_nodiff, t_yard, t_torch, agree), k in zip(SHAPES, calls, traced):
        pairs = L * (L + 1) // 2
        nbytes = n_out * N * L * 8
        k4 = sum(us for name, us in k.items() if name.startswith("k_p4_"))
        k2 = sum(us for name, us in k.items() if name.startswith("k_pilot_"))
        # per pair and sample: 2 LDS reads of 8 bytes; d_lo, d_hi 2 sub, pair sums 4 fma + 1 mul, t 3 sub, difference sums 3 fma +
        # 1 mul + 1 add = 15 FP64 instructions
        work = float(n_out) * N * pairs
        kp = k["k_p4_partial"] * 1e-6
        lines += ["", "N = %d, L = %d, n_out = %d: %d pairs, %.1f MB of values" % (N, L, n_out, pairs, nbytes / 1e6),
                  "  pilot_fourth_moments, whole call    %9.3f ms   (%.2f x pilot_statistics)" % (t_ours * 1e3, t_ours / t_yard),
                  "  ... without the difference sums     %9.3f ms" % (t_nodiff * 1e3),
                  "  its kernels alone                   %9.3f ms   (%.2f x the kernels of pilot_statistics; %s)"
                  % (k4 / 1e3, k4 / k2, ", ".join("%s %.1f us" % (n, us) for n, us in k.items() if n.startswith("k_p4_"))),
                  "  pilot_statistics, whole call        %9.3f ms" % (t_yard * 1e3),
                  "  its kernels alone                   %9.3f ms   (%s)"
                  % (k2 / 1e3, ", ".join("%s %.1f us" % (n, us) for n, us in k.items() if n.startswith("k_pilot_"))),
                  "  torch einsum formulation            %9.3f ms   (%.1f x pilot_fourth_moments; sums agree to %.1e)"
                  % (t_torch * 1e3, t_torch / t_ours, agree)]
        lines.append("  k_p4_partial                        %9.3f ms   (%.2f T FP64 instructions/s = %.0f %% of the vector rate of %.1f T/s; "
                     "%.1f TB/s of LDS reads)"
                     % (kp * 1e3, 15 * work / kp / 1e12, 100 * 15 * work / kp / (FP64_VECTOR_PEAK / 2), FP64_VECTOR_PEAK / 2e12,
                        16 * work / kp / 1e12))
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    if "--trace-child" in sys.argv:
        trace_child()
    else:
        main()

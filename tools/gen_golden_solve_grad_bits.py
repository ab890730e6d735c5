"""
Record what the fused solve + gradient kernel leaves (V, grad V, status, the v workspace; for the single-output update tail x, m,
V, status) on the plans of tests/solve_grad_bits_cases.py as the library of the CURRENT checkout computes them on the GPU, into
the .npz file named on the command line:

    python tools/gen_golden_solve_grad_bits.py OUT.npz

tests/golden/solve_grad_bits_parent.npz was recorded this way from the commit before k_solve_grad's prologue, fold addressing,
tile-wavefront addressing and the solver's prologue were rewritten; tests/test_gpu_solve_grad_bits.py holds every later build to
those bits.  The output path is mandatory and the tool refuses to write into tests/golden: the committed record is not to be
regenerated from newer code.  (To compare two builds, record each into a file of its own and compare the arrays.)
"""
import ctypes
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.join(ROOT, "tests"))


def v_peeker(plan):
    """() -> host copy of the plan's v workspace (n_out * n doubles), through the HIP runtime the process already has loaded"""
    import torch
    from bluest_amd._lib import check
    path = next(line.split()[-1] for line in open("/proc/self/maps") if "libamdhip64" in line)
    hip = ctypes.CDLL(path)
    hip.hipMemcpy.argtypes = [ctypes.c_void_p, ctypes.c_void_p, ctypes.c_size_t, ctypes.c_int]
    hip.hipMemcpy.restype = ctypes.c_int
    v = ctypes.c_void_p()
    check(plan.lib.bluest_plan_v_workspace(plan._h, ctypes.byref(v), None))

    def peek():
        torch.cuda.synchronize()
        out = np.empty(plan.n_out * plan.N, dtype=np.float64)
        assert hip.hipMemcpy(out.ctypes.data, v.value, out.nbytes, 2) == 0      # hipMemcpyDeviceToHost
        return out
    return peek


def main():
    import solve_grad_bits_cases as sgc
    from bluest_amd.plan import Plan
    if len(sys.argv) != 2:
        sys.exit("usage: python tools/gen_golden_solve_grad_bits.py OUT.npz")
    out = os.path.abspath(sys.argv[1])
    if os.path.dirname(out) == os.path.join(ROOT, "tests", "golden"):
        sys.exit("refusing to write into tests/golden: the committed record stays the parent commit's")
    data = {}
    for name in sgc.NAMES:
        p = sgc.problem(name)
        for k in sgc.ENV_KEYS:
            os.environ.pop(k, None)
        os.environ.update(p["env"])
        plan = Plan(p["n"], p["L"], p["outs"])
        cfg, lay = plan.launch_config(1), sgc.layout(p)
        for k in ("nt", "fused_tpb", "tiles_per_wg"):
            assert cfg[k] == lay[k], (name, k, cfg, lay)
        assert cfg["solve_grad_ku"] == lay["ku"] and cfg["matfree"] == 0, (name, cfg, lay)
        rec = sgc.record(plan, name, p, v_peeker(plan))
        data.update(rec)
        print("%-13s nt=%d ku=%d tiles_per_wg=%d/%d wgs=%s bpo=%d  status: %s" % (
            name, lay["nt"], lay["ku"], lay["tiles_per_wg"], lay["fused_tpb"], lay["wgs"], lay["bpo"],
            " ".join("%s=%s" % (k.split("/")[1], a.ravel().tolist()) for k, a in rec.items() if k.endswith("/st"))))
    np.savez(out, **data)
    print("wrote", out, os.path.getsize(out), "bytes")


if __name__ == "__main__":
    main()

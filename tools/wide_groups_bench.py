"""Measurements of the wide-group path, one JSON line per item:

  pinv     bluest_group_pinv for all 2^20 - 1 groups of n = 20 (device pointers: kernel time incl. the per-size launches)
  solve    SAP built directly over all groups of n = 20 (no clique enumeration): SAP / plan set-up, one evaluation step, cold
           and warm solve
  setup    BLUEProblem(20).setup_solver(K=20, eps) end to end: clique enumeration, SAP / plan set-up, solve, integer projection
  cliques  _Coupling.cliques(K) at M = 18 and 20 (host; complete and sparse coupling; median of 5 after one warm-up call)
  scratch  .private_segment_fixed_size of k_group_pinv_wide (compiled for gfx950 here; needs hipcc, no GPU)

    python tools/wide_groups_bench.py [pinv] [solve] [setup] [cliques] [scratch]
"""
import json
import os
import subprocess
import sys
import tempfile
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def emit(d):
    print(json.dumps(d), flush=True)


def bench_pinv(n=20, reps=3):
    import torch
    from bluest_amd import _lib, synth
    lib = _lib.lib()
    C, _ = synth.wishart_covariance(n)
    dC = torch.from_numpy(C).cuda()
    groups = synth.all_groups(n, n)
    dg = [torch.from_numpy(g).cuda() for g in groups]
    out = [torch.empty(len(g) * (k + 1) ** 2, dtype=torch.float64, device="cuda") for k, g in enumerate(groups)]
    per_k = {}
    for rep in range(reps + 1):
        torch.cuda.synchronize()
        t_all = time.perf_counter()
        for k in range(1, n + 1):
            t0 = time.perf_counter()
            _lib.check(lib.bluest_group_pinv(dC.data_ptr(), n, k, len(groups[k - 1]), dg[k - 1].data_ptr(), out[k - 1].data_ptr()))
            if rep > 0:
                per_k.setdefault(k, []).append((time.perf_counter() - t0) * 1e3)     # the call synchronises
        t_all = (time.perf_counter() - t_all) * 1e3
        if rep > 0:
            per_k.setdefault("all", []).append(t_all)
    emit({"item": "pinv", "n": n, "groups": int(2 ** n - 1), "ms_all_median": float(np.median(per_k["all"])),
          "ms_per_k_median": {str(k): round(float(np.median(per_k[k])), 4) for k in range(1, n + 1)},
          "ms_k17_20": round(float(sum(np.median(per_k[k]) for k in range(17, n + 1))), 4)})


def bench_solve(n=20):
    import torch
    from bluest_amd import synth
    from bluest_amd.sap import SAP
    C, _ = synth.wishart_covariance(n)
    w = np.concatenate([[1.0], 10.0 ** -np.linspace(1.0, 3.0, n - 1)])
    groups = synth.all_groups(n, n)
    costs = synth.group_costs(groups, w)
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    sap = SAP(C, n, [g.copy() for g in groups], costs, verbose=False)
    torch.cuda.synchronize()
    t_setup = time.perf_counter() - t0
    m = torch.from_numpy(np.full(len(costs), 1.0)).cuda()
    for _ in range(5):
        sap.plan.eval(m)
    torch.cuda.synchronize()
    steps = 50
    t0 = time.perf_counter()
    for _ in range(steps):
        sap.plan.eval(m)
    torch.cuda.synchronize()
    t_step = (time.perf_counter() - t0) / steps
    eps = float(np.sqrt(C[0, 0]) / 100.0)
    t0 = time.perf_counter()
    x = sap.solve(eps=eps, continuous_relaxation=True)
    t_cold = time.perf_counter() - t0
    t0 = time.perf_counter()
    x = sap.solve(eps=eps, continuous_relaxation=True)
    t_warm = time.perf_counter() - t0
    info = sap.solver_info
    emit({"item": "solve", "n": n, "K_tot": len(costs), "stored_bytes": int(sap.plan.phi_bytes + sap.plan.grad_bytes),
          "setup_s": round(t_setup, 3), "step_us": round(t_step * 1e6, 2), "solve_cold_s": round(t_cold, 4),
          "solve_warm_s": round(t_warm, 4), "method": info.get("method"), "certified_gap": info.get("certified_gap"),
          "support": int((x > 0).sum()), "widest_in_support": int(max(len(g) for g, xv in zip((tuple(r) for gk in groups for r in gk), x) if xv > 0))})


def bench_setup(n=20):
    from bluest_amd import BLUEProblem, synth
    from bluest_amd.blue_models import _Coupling
    C, _ = synth.wishart_covariance(n)
    w = np.concatenate([[1.0], 10.0 ** -np.linspace(1.0, 3.0, n - 1)])
    eps = float(np.sqrt(C[0, 0]) / 100.0)
    t0 = time.perf_counter()
    _Coupling(C, True).cliques(n)
    t_cl = time.perf_counter() - t0
    rows = []
    for rep in range(2):
        p = BLUEProblem(n, C=C.copy(), costs=w, verbose=False)
        t0 = time.perf_counter()
        d = p.setup_solver(K=n, eps=eps)
        rows.append(time.perf_counter() - t0)
    emit({"item": "setup_solver", "n": n, "K": n, "groups": int(2 ** n - 1), "cliques_s": round(t_cl, 3),
          "setup_solver_s": [round(r, 3) for r in rows], "total_cost": float(d["total_cost"]), "models_used": len(d["models"])})


def bench_cliques():
    from bluest_amd.blue_models import _Coupling
    for M in (18, 20):
        for kind in ("full", "sparse"):
            C = np.eye(M) + 0.5
            if kind == "sparse":
                C[1, 2] = C[2, 1] = 0.0          # one uncoupled pair: the clique enumeration proper
            cp = _Coupling(C, True)
            cp.cliques(M)
            ts = []
            for _ in range(5):
                t0 = time.perf_counter()
                out = cp.cliques(M)
                ts.append(time.perf_counter() - t0)
            emit({"item": "cliques", "M": M, "coupling": kind, "groups": int(sum(len(x) for x in out)),
                  "s_median": round(float(np.median(ts)), 3), "s_min": round(float(np.min(ts)), 3)})


def scratch_size():
    src = os.path.join(ROOT, "bluest_amd", "csrc", "mirrors.hip")
    with tempfile.TemporaryDirectory() as d:
        asm = os.path.join(d, "mirrors.s")
        subprocess.check_call(["hipcc", "--offload-arch=gfx950", "-O3", "-std=c++17", "--cuda-device-only", "-S",
                               "-I" + os.path.join(ROOT, "include"), "-I" + os.path.join(ROOT, "bluest_amd", "csrc"), src, "-o", asm])
        text = open(asm).read()
    res, cur = {}, None
    for line in text.splitlines():
        s = line.strip()
        if s.startswith(".name:") or s.startswith("- .name:") or ".name:" in s:
            nm = s.split(".name:")[1].strip()
            cur = nm if "k_group_pinv_wide" in nm else None
        if cur and ".private_segment_fixed_size:" in s:
            res[cur] = int(s.split(":")[1])
            cur = None
    emit({"item": "scratch", "private_segment_fixed_size": res})


if __name__ == "__main__":
    what = sys.argv[1:] or ["pinv", "solve", "setup", "cliques", "scratch"]
    for w_ in what:
        {"pinv": bench_pinv, "solve": bench_solve, "setup": bench_setup, "cliques": bench_cliques, "scratch": scratch_size}[w_]()

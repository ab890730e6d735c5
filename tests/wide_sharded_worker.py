"""
Worker of tests/test_gpu_wide_groups.py::test_sharded_two_ranks_wide_groups (launched with torch.distributed.run, one process per
rank, all ranks on cuda:0 with the gloo backend).  Group-sharded HIP plans (bluest_amd/dist.py) over a group set with groups of
17..24 models: the sharded evaluation against the single-process plan, and the sharded solve (sharded multiplicative phase,
collective column generation, redundant masters over replicated sub-plans of the support); rank 0 writes the results.
"""
import json
import os
import sys

import numpy as np
import torch
import torch.distributed as dist

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bluest_amd.dist import ShardedPlan, sharded_spg   # noqa: E402
from bluest_amd.plan import Plan                  # noqa: E402


def problem(n, n_out, seed=1, n_wide=30, wide=(17, 24)):
    """one-factor covariances (cheap, individually poor models that pay in wide groups), singletons, pairs, random wide
    groups and the full group; groups ordered by size, then lexicographic"""
    rng = np.random.RandomState(seed)
    Cs = [np.ones((n, n)) + np.diag(np.concatenate([[0.01], rng.uniform(0.5, 2.0, n - 1)])) for _ in range(n_out)]
    w = np.concatenate([[1.0], 10.0 ** -rng.uniform(2.0, 3.0, n - 1)])
    gl = [(i,) for i in range(n)] + [(i, j) for i in range(n) for j in range(i + 1, n)]
    wide_g = set()
    while len(wide_g) < n_wide:
        wide_g.add(tuple(sorted(rng.choice(n, rng.randint(wide[0], min(wide[1], n) + 1), replace=False).tolist())))
    gl = sorted(set(gl) | wide_g | {tuple(range(n))}, key=lambda g: (len(g), g))
    K = max(len(g) for g in gl)
    levels = [np.array([g for g in gl if len(g) == k], dtype=np.int64).reshape(-1, k) for k in range(1, K + 1)]
    costs = np.array([w[list(g)].sum() for g in gl])
    return Cs, levels, costs, K


def main(out_path):
    torch.cuda.set_device(0)
    dev = torch.device("cuda", 0)
    dist.init_process_group("gloo")
    rank, world = dist.get_rank(), dist.get_world_size()
    res = {"world": world}
    for tag, (n, n_out) in (("n24_o1", (24, 1)), ("n20_o2", (20, 2))):
        Cs, levels, costs, K = problem(n, n_out)
        sizes = [len(x) for x in levels]
        L = int(sum(sizes))
        outs = [{"K": K, "sizes": sizes, "groups": levels, "C": Cs[o], "mapping": None} for o in range(n_out)]
        sp = ShardedPlan(n, sizes, outs, device=dev)
        full = Plan(n, L, outs, device=dev)
        m = torch.from_numpy(np.random.RandomState(3).rand(L) * 10.0 + 0.5).to(dev)
        var, grad_local, status = sp.eval(m)
        v_full, g_full, st_full = full.eval(m)
        coef = torch.from_numpy(np.linspace(0.5, 1.0, n_out).reshape(1, -1)).to(dev)
        g_glob = sp.combine_grad(grad_local, coef)
        g_want = full.combine_grad(g_full, coef)
        res[tag + "_eval_err"] = float((var / v_full - 1).abs().max())
        res[tag + "_grad_err"] = float((g_glob - g_want).abs().max() / g_want.abs().max())
        res[tag + "_status_equal"] = bool(torch.equal(status, st_full))
        res[tag + "_shard"] = [sp.lo, sp.hi]
        res[tag + "_L"] = L
        res[tag + "_wide_first"] = int(sum(sizes[:16]))
        B = 50.0 * float(costs[:n].sum())
        m_sh, info = sharded_spg(sp, costs, budget=B)
        all_m = [torch.empty(L, dtype=torch.float64) for _ in range(world)]
        dist.all_gather(all_m, torch.from_numpy(np.ascontiguousarray(m_sh)))
        res[tag + "_ranks_agree"] = bool(all(torch.equal(all_m[0], q) for q in all_m))
        vs, _, _ = full.eval(torch.from_numpy(m_sh).to(dev), want_grad=False)
        res[tag + "_F_sharded"] = float(vs.max())
        res[tag + "_cost_ratio"] = float(m_sh @ costs / B)
        res[tag + "_method"] = info.get("method", "spg")
        res[tag + "_gap"] = float(info.get("certified_gap", np.nan))
        res[tag + "_wide_in_support"] = int((m_sh[res[tag + "_wide_first"]:] > 0).sum())
        # the single-GPU answer of the same problem
        from bluest_amd.colgen import colgen_solve
        x1, i1 = colgen_solve(full, costs, np.ones(n_out), B)
        v1, _, _ = full.eval(torch.from_numpy(B / costs * x1).to(dev), want_grad=False)
        res[tag + "_F_single"] = float(v1.max())
    if rank == 0:
        json.dump(res, open(out_path, "w"))
    dist.destroy_process_group()


if __name__ == "__main__":
    main(sys.argv[1])

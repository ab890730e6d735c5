"""
Second-order finish of solver="spg" on the GPU (C-ABI Part 6, csrc/newton.hip): multiplicative phase on all groups, then
column generation with a Newton master on the support and a certified duality gap from every pricing round.

The reference passes this problem -- min_m max_o V_o(m)/s_o s.t. cost.m = B, m >= 0 -- to third-party NLP solvers together with
the Hessian of bluest/misc.py:497-503 (bluest/sap.py:387-456, bluest/mosap.py:578-673); none of them is available to this
build, and a first-order method alone needs ~1300 iterations and leaves a residual of a few 1e-6.

Everything numeric runs in hand-written kernels; the host only moves a few KB per round (the support's values, the
multipliers, 1024 pricing candidates) and decides which groups enter.  torch is used for buffers and the stream only.
"""
import ctypes

import numpy as np
import torch

from ._lib import BluestHipError, check
from .plan import EVAL_OK, _stream

MASTER_OUT = 16            # layout of the master's result record (include/bluest_hip.h, bluest_master_newton)
N_CAND = 1024              # BLUEST_PRICE_CANDIDATES


class _Buffers(object):
    """ONE device buffer for everything the host reads back per round, so that a round costs one device-to-host copy"""

    def __init__(self, dev, n_out, s_max):
        self.n_out, self.s_max = n_out, s_max
        sizes = [("out", MASTER_OUT + n_out), ("xs", s_max), ("mu", n_out), ("var", n_out), ("y0", n_out), ("csup", s_max), ("topv", N_CAND), ("topi", N_CAND)]
        self.off, tot = {}, 0
        for name, n in sizes:
            self.off[name] = (tot, n)
            tot += n
        self.buf = torch.from_numpy(np.zeros(tot)).to(dev)
        self.base = self.buf.data_ptr()

    def ptr(self, name):
        return self.base + 8 * self.off[name][0]

    def fetch(self):
        h = self.buf.cpu().numpy()
        out = {name: h[o:o + n] for name, (o, n) in self.off.items()}
        out["topi"] = out["topi"].view(np.int64)
        return out

    def put(self, name, values):
        o, n = self.off[name]
        v = np.zeros(n)
        v[:len(values)] = values
        self.buf[o:o + n] = torch.from_numpy(v)          # small H2D copy (slice assignment from a CPU tensor: a memcpy)

    def put_xs_mu(self, xs, mu):
        """the master's two inputs in ONE copy (they are neighbours in the buffer)"""
        (o, n), (o2, n2) = self.off["xs"], self.off["mu"]
        assert o2 == o + n
        v = np.zeros(n + n2)
        v[:len(xs)] = xs
        v[n:n + len(mu)] = mu
        self.buf[o:o + n + n2] = torch.from_numpy(v)


def top_candidates(topv, topi, k):
    """the k best pricing candidates, largest reduced cost first, ties by index -- the head of np.lexsort((topi, -topv)) without sorting
    all 1024 (56 us and two 1024-entry tolist() per round on the host while the GPU waits)"""
    if k < len(topv):
        head = np.argpartition(-topv, k)[:k]
        kth = topv[head].min()
        head = np.flatnonzero(topv >= kth)                        # every tie of the k-th value comes along: same head as the full sort
    else:
        head = np.arange(len(topv))
    o = np.lexsort((topi[head], -topv[head]))
    return topi[head][o].tolist(), topv[head][o].tolist()


def _fused_ma_ok(plan):
    """the plan's widest group is within what bluest_plan_eval_ma accepts on it (both read from the plan)"""
    lim, km = ctypes.c_int(0), ctypes.c_int(0)
    check(plan.lib.bluest_plan_eval_ma_kmax(plan._h, ctypes.byref(lim)))
    check(plan.lib.bluest_plan_kmax(plan._h, ctypes.byref(km)))
    return 0 < km.value <= lim.value


def master_max_support(plan):
    s = ctypes.c_int(0)
    with torch.cuda.device(plan.device):
        check(plan.lib.bluest_master_max_support(plan._h, ctypes.byref(s)))
    return int(s.value)


def cap_feasible_start(x, Acap, b):
    """a point of the simplex that respects Acap x <= b, made from x by scaling the entries of the most violated cap's groups down
    (with 5 % room) and handing the freed mass to the entries outside that cap; None if that does not terminate (e.g. every
    entry is capped)"""
    x = np.maximum(np.asarray(x, dtype=np.float64), 0.0)
    x = x / x.sum()
    for _ in range(500):
        viol = Acap @ x - b
        if (viol <= 0.0).all():
            return x
        c = int(np.argmax(viol / np.maximum(b, 1e-300)))
        msk = Acap[c] > 0.0
        rest = float(x[~msk].sum())
        if rest <= 0.0 or b[c] <= 0.0:
            return None
        x[msk] *= 0.95 * b[c] / float(Acap[c] @ x)
        x[~msk] *= (1.0 - float(x[msk].sum())) / rest
    return None


def colgen_solve(plan, costs, s, B, x0=None, prm=None, log=None, caps=None):
    """x (numpy, length L, on the unit simplex) minimising max_o V_o(B x / cost)/s_o, and an info dict with the certified gap.
    Returns (None, reason) when the master problem does not fit the single-workgroup kernel (the caller falls back).

    plan: a plan.Plan, or a dist.ShardedPlan (COLLECTIVE: every rank of the group calls this with the same arguments).  Over a
    sharded group set nothing of length K_tot ever crosses the fabric: the allocation, the gradient and the multiplicative
    iterate stay sharded (every rank updates the entries of its own groups); per evaluation the ranks exchange the Phi records
    (n_out (N^2 + 2N + 1) doubles, dist.ShardedPlan.reduce_records) and solve redundantly; per pricing round they gather
    <= 1024 candidates and the blocks of the <= 64 support groups; the master problem is solved redundantly by every rank with
    the same deterministic kernel, so all ranks take identical decisions and return identical bits.

    caps (single GPU): {"models": int array (n_caps), "rows": (n_caps, L) 0/1 indicator of the groups containing each capped model,
    "rhs": (n_caps) maximal numbers of samples} -- max_model_samples (bluest/sap.py:222-240, bluest/mosap.py:326-344):
    sum_i rows[c, i] m_i <= rhs[c].  The caps are linear rows of the master's KKT system (bluest_master_newton_capped), the pricing
    subtracts their multipliers (bluest_price_capped) and the bound becomes  A - max_i c^_i - sum_c nu'_c rhs_c  (Lagrangian
    relaxation of the caps, multipliers nu' = F^2 nu of the problem as posed)."""
    prm = prm or {}
    sharded = plan if hasattr(plan, "reduce_records") else None
    if sharded is not None and caps is not None:
        return None, "sample caps over a sharded plan are not supported"
    if sharded is not None:
        plan = sharded.plan
    world = 1 if sharded is None else sharded.world
    ma_its = int(prm.get("ma_iterations", 200))
    ma_p = float(prm.get("ma_p", 32.0))
    init_mult = int(prm.get("support_init", 3))
    eps_list = tuple(prm.get("background", (1.0e-3, 1.0e-6)))
    gap_tol = float(prm.get("gap_tol", 1.0e-7))
    enter_tol = float(prm.get("enter_tol", 1.0e-8))
    max_rounds = int(prm.get("max_rounds", 60))
    newton_maxit = int(prm.get("newton_maxit", 60))
    lib, dev = plan.lib, plan.device
    L, N, n_out = plan.L, plan.N, plan.n_out
    w = np.asarray(costs, dtype=np.float64)
    s = np.asarray(s, dtype=np.float64)
    s_max = master_max_support(plan)
    enter_per = int(prm.get("enter_per_round", N))
    if n_out > 64:
        return None, "more than 64 outputs"
    if s_max < min(L, N + 8):
        return None, "master problem does not fit one workgroup (support limit %d)" % s_max

    def to_dev(a, dtype=np.float64):
        return torch.from_numpy(np.ascontiguousarray(a, dtype=dtype)).to(dev)

    import time as _time
    host_ms = {} if prm.get("profile") else None         # prm["profile"]: host wall-clock per segment of this function (info["host_ms"])
    _last = [_time.perf_counter()]

    def lap(name):
        if host_ms is not None:
            now = _time.perf_counter()
            host_ms[name] = host_ms.get(name, 0.0) + (now - _last[0]) * 1e3
            _last[0] = now

    cc_h = B / w
    cc, s_d = to_dev(cc_h), to_dev(s)
    ncap = 0
    if caps is not None:
        cap_models = np.ascontiguousarray(caps["models"], dtype=np.int32)
        cap_rows = np.asarray(caps["rows"]) != 0
        cap_rhs = np.ascontiguousarray(caps["rhs"], dtype=np.float64)
        ncap = len(cap_models)
        if ncap > 64 or cap_rows.shape != (ncap, L):
            return None, "more than 64 sample caps"
        cap_asum = np.array([float(cc_h[cap_rows[c]].sum()) for c in range(ncap)])      # cap c of the uniform allocation is asum / L
        mask = np.zeros(L, dtype=np.uint64)
        for c in range(ncap):
            mask[cap_rows[c]] |= np.uint64(1) << np.uint64(c)
        capmask_d = torch.from_numpy(mask.view(np.int64)).to(dev)
        nu_d = torch.zeros(64, dtype=torch.float64, device=dev)

        def cap_system(keep_idx, eps_):
            """(rows of the caps on the support in the master's variable, right-hand sides with the background's share taken off)"""
            return (1.0 - eps_) * cc_h[keep_idx][None, :] * cap_rows[:, keep_idx], cap_rhs - eps_ * cap_asum / L
    bufs = _Buffers(dev, n_out, s_max)
    var = torch.empty((1, n_out), dtype=torch.float64, device=dev)
    grad = torch.empty((1, plan.grad_len), dtype=torch.float64, device=dev)
    status = torch.empty((1, n_out), dtype=torch.int32, device=dev)
    info = {"rounds": 0, "newton_it": 0, "master_evals": 0, "full_evals": 0, "ma_iterations": ma_its, "ranks": world}
    var_view = bufs.buf[bufs.off["var"][0]:bufs.off["var"][0] + n_out].view(1, n_out)
    rec = torch.empty((1, n_out, plan.reclen), dtype=torch.float64, device=dev) if sharded is not None else None

    def gather(obj):
        """list over ranks of `obj` (small host data)"""
        if world == 1:
            return [obj]
        import torch.distributed as dist
        got = [None] * world
        dist.all_gather_object(got, obj, group=sharded.group)
        return got

    def evaluate(m_t, var_t):
        """V and grad V of the allocation m_t for every output into (var_t, grad, status), on the stream"""
        if sharded is None:
            check(lib.bluest_plan_eval(plan._h, m_t.data_ptr(), 1, L, 0.0, var_t.data_ptr(), grad.data_ptr(), plan.grad_len, status.data_ptr(), st))
        else:
            sharded.eval(m_t, rec=rec, out=(var_t, grad, status))       # Phi of the shard -> record exchange -> redundant solve + shard gradient

    with torch.cuda.device(dev):
        st = _stream()
        # ---- background: Phi_o(uniform allocation), one Phi pass -----------------------------------------------------
        u_m = to_dev(cc_h / L)
        rec_u = plan.phi(u_m)
        if sharded is not None:
            sharded.reduce_records(rec_u)
        info["full_evals"] += 1                                  # (fetched after phase 1: its launches do not wait for this round trip)
        # ---- phase 1: multiplicative algorithm from the uniform point (or x0) ------------------------------------------------
        xh = np.full(L, 1.0 / L) if x0 is None else np.maximum(np.asarray(x0, dtype=np.float64), 0.0)
        xh = xh / xh.sum()
        if x0 is not None:
            xh = (1.0 - 1.0e-3) * xh + 1.0e-3 / L                # the multiplicative update cannot leave a zero
        x_d, m_d = to_dev(xh), to_dev(cc_h * xh)
        lap("background")
        _t_ma0 = _time.perf_counter()
        # a single output on all groups: the fused solve + gradient kernel of the evaluation applies the update itself (two launches
        # per step instead of three, no gradient array; the same iterates bit for bit)
        # (only while the plan's widest group is within what that kernel's tail handles: the plan reports both)
        fused_ma = sharded is None and n_out == 1 and bool(getattr(plan, "identity", False)) and _fused_ma_ok(plan)
        for _ in range(ma_its):
            if fused_ma:
                check(lib.bluest_plan_eval_ma(plan._h, m_d.data_ptr(), var.data_ptr(), status.data_ptr(), s_d.data_ptr(), cc.data_ptr(), x_d.data_ptr(), st))
                continue
            evaluate(m_d, var)
            check(lib.bluest_ma_update(plan._h, var.data_ptr(), status.data_ptr(), grad.data_ptr(), s_d.data_ptr(), cc.data_ptr(), ma_p,
                                       x_d.data_ptr(), m_d.data_ptr(), st))
        info["full_evals"] += ma_its
        lap("ma launches")
        xh = x_d.cpu().numpy()
        rec_u = rec_u.cpu().numpy()[0]                           # (n_out, N*N + 2N + 1): the sums come first
        phi_u = np.ascontiguousarray(rec_u[:, :N * N])
        lap("ma wait + fetch")
        info["t_ma_ms"] = (_time.perf_counter() - _t_ma0) * 1e3
        _t_r0 = _time.perf_counter()
        S0 = min(L, s_max, max(init_mult * N, N + 1))
        if sharded is not None:
            # every rank owns the entries of its groups; the others never moved (or were zeroed by the first update)
            own = np.zeros(L, dtype=bool)
            for o_ in sharded.local_outputs:
                own[np.asarray(o_["mapping"], dtype=np.int64)] = True
            xh = np.where(own, xh, 0.0)
            mine = np.flatnonzero(own)                            # only owned entries travel (a rank with fewer than S0 groups
            top = mine[np.argsort(-xh[mine], kind="stable")[:S0]]  # would otherwise offer indices it does not own, at value 0)
            parts = gather((top, xh[top]))
            idx_all = np.concatenate([p_[0] for p_ in parts])
            val_all = np.concatenate([p_[1] for p_ in parts])
            if not np.isfinite(val_all).all() or val_all.sum() <= 0.0:
                return None, "multiplicative phase produced a non-finite iterate"
            order = np.lexsort((idx_all, -val_all))[:S0]       # largest first, ties by index: the same on every rank
            order = order[val_all[order] > 0.0]                # the master wants a strictly ascending support of positive entries
            keep, first = np.unique(idx_all[order], return_index=True)
            xs = val_all[order][first]
            xs = xs / xs.sum()
        else:
            if not np.isfinite(xh).all() or xh.sum() <= 0.0:
                return None, "multiplicative phase produced a non-finite iterate"
            xh = np.maximum(xh, 0.0) / xh.sum()
            # ---- initial support: the largest entries -----------------------------------------------------------------------
            keep = np.sort(np.argpartition(-xh, S0 - 1)[:S0] if S0 < L else np.arange(L))     # O(L) selection (a full sort of
            xs = xh[keep] / xh[keep].sum()                                                       # 245505 entries costs 15-25 ms)
        lap("initial support")
        mu = np.full(n_out, 1.0 / n_out)
        best_lb, F_last, gap, cert = 0.0, np.inf, np.inf, None
        x_full = None
        sup_d = torch.empty(s_max, dtype=torch.int64, device=dev)

        def master_plan(keep_idx):
            """(plan holding the blocks of the support groups, their indices in that plan).  Sharded: the blocks live on the ranks
            that own the groups, so a small plan over exactly the support is assembled identically on every rank (collective)"""
            if sharded is None:
                return plan, keep_idx
            sub = sharded.replicated_subplan(keep_idx)            # raises on every rank alike if an output would be left empty
            subs.append(sub)                                      # alive until the master kernel that reads it has run
            return sub, np.arange(len(keep_idx), dtype=np.int64)
        subs = []
        # the stages of eps_list, the polish and the certificate; when that certificate is short of tight_gap, ONE more stage under a
        # background of tight_background (1e-9) and the polish + certificate again (measured: profiles/r04_gap_table.txt)
        stage_list, stage_next = list(eps_list), 0
        tight_eps, tight_gap = float(prm.get("tight_background", 1.0e-9)), float(prm.get("tight_gap", 1.0e-10))
        while True:
            for stage in range(stage_next, len(stage_list)):
                eps = stage_list[stage]
                bg_d = to_dev(eps * phi_u)
                mtol = 1.0e-2
                for rnd in range(max_rounds):
                    S = len(keep)
                    if ncap:
                        Acap_S, b_eps = cap_system(keep, eps)
                        if (Acap_S @ xs > b_eps).any():            # first round of a stage (the background's share changed) or a fresh support
                            xs = cap_feasible_start(xs, Acap_S, b_eps)
                            if xs is None:
                                return None, "no allocation on the support respects the sample caps"
                    bufs.put_xs_mu(xs, mu)
                    keep_h = np.ascontiguousarray(keep, dtype=np.int64)
                    cc_keep = np.ascontiguousarray(cc_h[keep])
                    mplan, msup = master_plan(keep_h)
                    lap("round: stage inputs")
                    try:
                        if ncap:
                            b_host = np.ascontiguousarray(b_eps)
                            check(lib.bluest_master_newton_capped(mplan._h, S, msup.ctypes.data, cc_keep.ctypes.data, s_d.data_ptr(), bg_d.data_ptr(),
                                                                  float(eps), bufs.ptr("xs"), bufs.ptr("mu"), float(mtol), newton_maxit, bufs.ptr("out"),
                                                                  ncap, cap_models.ctypes.data, b_host.ctypes.data, nu_d.data_ptr(), st))
                        else:
                            check(lib.bluest_master_newton(mplan._h, S, msup.ctypes.data, cc_keep.ctypes.data, s_d.data_ptr(), bg_d.data_ptr(), float(eps),
                                                           bufs.ptr("xs"), bufs.ptr("mu"), float(mtol), newton_maxit, bufs.ptr("out"), st))
                    except BluestHipError as err:                     # e.g. the LDS attribute refused on this device: the caller falls back
                        return None, "master launch failed (%s)" % err
                    lap("round: master launch")
                    sup_d[:S] = torch.from_numpy(keep_h)
                    check(lib.bluest_support_point(L, S, sup_d.data_ptr(), bufs.ptr("xs"), cc.data_ptr(), float(eps), m_d.data_ptr(), st))
                    evaluate(m_d, var_view)
                    if ncap:
                        check(lib.bluest_price_capped(plan._h, grad.data_ptr(), bufs.ptr("mu"), s_d.data_ptr(), cc.data_ptr(), S, sup_d.data_ptr(),
                                                      bufs.ptr("csup"), bufs.ptr("topv"), bufs.ptr("topi"), bufs.ptr("y0"),
                                                      capmask_d.data_ptr(), nu_d.data_ptr(), bufs.ptr("out"), st))
                    else:
                        check(lib.bluest_price(plan._h, grad.data_ptr(), bufs.ptr("mu"), s_d.data_ptr(), cc.data_ptr(), S, sup_d.data_ptr(),
                                               bufs.ptr("csup"), bufs.ptr("topv"), bufs.ptr("topi"), bufs.ptr("y0"), st))
                    lap("round: eval + price launches")
                    h = bufs.fetch()                                  # the round's only synchronisation
                    lap("round: wait + fetch")
                    nu_h = nu_d.cpu().numpy()[:ncap] if ncap else None
                    if sharded is not None:
                        # every rank priced its own groups: merge the candidates and the support's reduced costs (a rank reports 0
                        # for groups it does not own; reduced costs are >= 0).  Same data, same order on every rank.
                        parts = gather((h["topv"], h["topi"], h["csup"][:S]))
                        h["topv"] = np.concatenate([p_[0] for p_ in parts])
                        h["topi"] = np.concatenate([p_[1] for p_ in parts])
                        h["csup"] = np.max(np.stack([p_[2] for p_ in parts]), axis=0)
                    out = h["out"]
                    info["rounds"] += 1
                    info["newton_it"] += int(out[4])
                    info["master_evals"] += int(out[5])
                    info["full_evals"] += 1
                    info["master_solves"] = info.get("master_solves", 0) + int(out[6])
                    if int(out[7]) == 2 or not np.isfinite(out[0]):
                        return None, "master start not evaluable"
                    xs, mu = h["xs"][:S].copy(), h["mu"].copy()
                    F = float(out[0])
                    pos = xs > 0.0
                    # certified bound (valid for ANY multipliers / vectors: weak duality), budget 1 in the scaled variable
                    a = mu / s
                    A = 2.0 * float(a @ h["y0"])                      # y_{o,0} of the vectors the c_i were taken with (NOT V: see k_price)
                    cmax = max(float(h["topv"].max()), float(h["csup"][:S].max()))
                    lb = A * A / (4.0 * cmax) if cmax > 0.0 else 0.0
                    if ncap:                                          # Lagrangian relaxation of the caps (multipliers F^2 nu >= 0: any are valid)
                        lb = max(A - cmax - float(out[0]) ** 2 * float(nu_h @ cap_rhs), 0.0)
                    if lb > best_lb:                                  # the point + multipliers the bound was obtained at: a certificate
                        best_lb = lb                                  # anybody can re-evaluate (tests do, with the CPU checker)
                        cert = {"support": keep.copy(), "x": xs.copy(), "mu": mu.copy(), "background": float(eps), "lower_bound": lb}
                        if ncap:
                            cert["cap_multipliers"] = float(out[0]) ** 2 * nu_h
                    gap = 1.0 - best_lb / F
                    level = float(h["csup"][:S][pos] @ xs[pos]) / float(xs[pos].sum())
                    in_pos = set(keep[pos].tolist())
                    enter = []
                    room = s_max - int(pos.sum())
                    cand_i, cand_v = top_candidates(h["topv"], h["topi"], min(enter_per, room) + len(in_pos) + 1)      # largest first, ties by index
                    for i, v in zip(cand_i, cand_v):
                        if len(enter) >= min(enter_per, room) or i < 0 or v / level - 1.0 <= enter_tol:
                            break
                        if i not in in_pos:
                            enter.append(i)
                    if log is not None:
                        log("eps %.0e round %2d F_eps %.12e gap %.3e |S| %3d nnz %3d newton %2d evals %3d enter %3d kkt %.1e status %d"
                            % (eps, rnd, F, gap, S, int(pos.sum()), int(out[4]), int(out[5]), len(enter), out[2], int(out[7])))
                    x_full = (keep[pos], xs[pos] / xs[pos].sum())
                    F_last = F
                    lap("round: host decisions")
                    nudge = 0.0
                    if int(out[7]) == 1 and int(out[4]) == 0 and rnd > 0:
                        # the master cannot move from here (stalled): pricing again would offer the same columns.  While the certified
                        # gap is not met and columns still want to enter, let them enter with a little mass instead of zero (a column
                        # at zero is where the master's quadratic model is least trustworthy) -- a few times per stage, then give up
                        nudges = info.setdefault("nudges", [0] * (len(eps_list) + 1))
                        if gap <= gap_tol or len(enter) == 0 or nudges[stage] >= 3:
                            break
                        nudges[stage] += 1
                        nudge = 1.0e-3 * float(xs[pos].mean())
                    if len(enter) == 0:
                        # (going on to the next stage without the tight solve of this one saves a round or two on the synthetic problems but
                        # leaves the ill-conditioned Navier-Stokes problem with a stalled first master of the next stage: measured, not kept)
                        if mtol > 1.0e-9:
                            mtol = 1.0e-9                              # the support is priced out at a loose master: tighten once
                            keep, xs = keep[pos], xs[pos] / xs[pos].sum()
                            continue
                        break
                    viol = cand_v[0] / level - 1.0
                    mtol = max(1.0e-9, min(1.0e-2, 1.0e-2 * float(viol)))
                    new_keep = np.concatenate([keep[pos], np.asarray(enter, dtype=np.int64)])
                    new_x = np.concatenate([xs[pos], np.full(len(enter), nudge)])   # enter at zero: the master frees them (reduced cost < 0)
                    o2 = np.argsort(new_keep, kind="stable")
                    keep, xs = new_keep[o2], new_x[o2] / new_x.sum()
                    if gap <= gap_tol and stage == len(stage_list) - 1:
                        pass                                           # keep pricing until no column enters: cheap, and it lowers F
            # ---- polish on the final support without background (the function the reference evaluates) --------------------------
            lap("round: host decisions")
            stage_end = (x_full[0], x_full[1], mu)
            # Entries below the last stage's background are, with few exceptions, the ones the polish would spend a dozen iterations
            # driving out: they are taken out BEFORE the first polish, and the certificate decides -- a gap above 0.1 x that background
            # says something the optimum needs went with them (30 models / 4 outputs, 48 / 1: 1e-6), and the polish starts over with
            # all entries.  BASELINE configurations: same certified gaps, 0.7 .. 1.8 ms less (profiles/r04_gap_table.txt)
            pre = float(prm.get("pretrim", 1.0)) * stage_list[-1]
            for use_pre in ((True, False) if (pre > 0.0 and not ncap) else (False,)):
                keep, xs, mu = stage_end
                info["polished"] = False
                if use_pre:
                    small = xs < pre
                    if not small.any() or small.all():
                        continue
                    keep, xs = keep[~small], xs[~small] / float(xs[~small].sum())
                for polish_pass in range(int(prm.get("polish_passes", 3))):
                    S = len(keep)
                    keep_h = np.ascontiguousarray(keep, dtype=np.int64)
                    cc_keep = np.ascontiguousarray(cc_h[keep])
                    # (entries on their way out shrink by the factor 10 per iteration: a dozen iterations show them; a polish that
                    # converges needs 3 to 5)
                    pol_maxit = newton_maxit if (ncap or polish_pass > 0) else min(newton_maxit, 12)
                    mplan, msup = master_plan(keep_h)
                    if ncap:
                        Acap_S, b0 = cap_system(keep, 0.0)
                        start = cap_feasible_start(xs, Acap_S, b0) if (Acap_S @ xs > b0).any() else xs
                        if start is None:
                            return None, "no allocation on the final support respects the sample caps"
                        xs = start
                    bufs.put("xs", xs)
                    bufs.put("mu", mu)
                    sup_d[:S] = torch.from_numpy(keep_h)
                    fin_var = torch.empty((2, 1, n_out), dtype=torch.float64, device=dev)
                    fin_st = torch.empty((2, 1, n_out), dtype=torch.int32, device=dev)

                    def eval_support(which):
                        """the truth: F of the sparse allocation itself (support vector in the round buffer, no background), evaluated by the
                        plan on the stream -- nothing of length K_tot crosses PCIe"""
                        check(lib.bluest_support_point(L, S, sup_d.data_ptr(), bufs.ptr("xs"), cc.data_ptr(), 0.0, m_d.data_ptr(), st))
                        (sharded if sharded is not None else plan).eval(m_d, want_grad=False, out=(fin_var[which], None, fin_st[which]))
                    eval_support(0)                                           # before the polish ...
                    try:
                        if ncap:
                            b_host = np.ascontiguousarray(b0)
                            check(lib.bluest_master_newton_capped(mplan._h, S, msup.ctypes.data, cc_keep.ctypes.data, s_d.data_ptr(), None, 0.0, bufs.ptr("xs"),
                                                                  bufs.ptr("mu"), 1.0e-10, pol_maxit, bufs.ptr("out"), ncap, cap_models.ctypes.data,
                                                                  b_host.ctypes.data, nu_d.data_ptr(), st))
                        else:
                            check(lib.bluest_master_newton(mplan._h, S, msup.ctypes.data, cc_keep.ctypes.data, s_d.data_ptr(), None, 0.0,
                                                           bufs.ptr("xs"), bufs.ptr("mu"), 1.0e-10, pol_maxit, bufs.ptr("out"), st))
                    except BluestHipError as err:
                        return None, "master launch failed (%s)" % err
                    eval_support(1)                                           # ... and after it (a support vector the master could not evaluate stays as it was)
                    h = bufs.fetch()
                    fv, fs = fin_var.cpu().numpy()[:, 0], fin_st.cpu().numpy()[:, 0]
                    out = h["out"]
                    info["newton_it"] += int(out[4])
                    info["master_evals"] += int(out[5])
                    info["full_evals"] += 2

                    def value(which):
                        return float((fv[which] / s).max()) if (fs[which] == EVAL_OK).all() else np.inf
                    F_start = value(0)
                    info["polish"] = {"support": S, "status": int(out[7]), "newton_it": int(out[4]), "kkt": float(out[2]), "F_before": F_start, "F_master": float(out[0])}
                    info.setdefault("polish_passes", []).append(info["polish"])
                    if polish_pass == 0:
                        best_pt, F_true = (keep, xs, mu), F_start
                    elif F_start <= F_true * (1.0 + 1.0e-8):
                        # this pass starts from the previous master's point with its vanishing entries taken out (below).  The point it is
                        # compared with has entries down to 1e-9 of the largest: it is evaluated on an ill-conditioned matrix, to about
                        # 1e-9 (profiles/r04_optimum_floor.txt), so the clean point is not refused over less than that
                        best_pt, F_true = (keep, xs, mu), F_start
                        info["polished"] = True
                    else:
                        break
                    xm, mum = h["xs"][:S].copy(), h["mu"].copy()
                    if int(out[7]) != 2 and np.isfinite(out[0]):
                        F_pol = value(1)
                        if ncap and (cap_system(keep, 0.0)[0] @ np.maximum(xm, 0.0) > cap_rhs * (1.0 + 1.0e-9)).any():
                            F_pol = np.inf
                        if F_pol < F_true:
                            best_pt, F_true = (keep, xm, mum), F_pol
                            info["polished"] = True
                        # without the background an entry the optimum does not use can only shrink geometrically inside the master (it
                        # keeps every model in the information matrix: V has a kink where one drops out), and once the only groups that
                        # sample some model are down at 1e-30 the matrix is too ill-conditioned for the master's own KKT measure: it stalls
                        # a few 1e-9 short.  Take those entries out and polish again on what is left (models nothing samples leave the
                        # system, as they do in the reference's evaluation); the pricing below judges the result like any other point
                        tiny = np.maximum(xm, 0.0) < 1.0e-12 * float(xm.max())
                        unresolved = int(out[7]) == 1 or float(out[2]) > 1.0e-8                    # stalled, or out of iterations short of the KKT point
                        if not ncap and unresolved and np.isfinite(F_pol) and not tiny.all() and (tiny.any() or polish_pass == 0):
                            keep, xs, mu = keep[~tiny], xm[~tiny] / float(xm[~tiny].sum()), mum
                            continue
                    break
                keep, xs, mu = best_pt
                S = len(keep)
                sup_d[:S] = torch.from_numpy(np.ascontiguousarray(keep, dtype=np.int64))
                # ---- one more pricing, AT THE RETURNED POINT, under a background of 1e-9: the bound of the last stage was taken at that
                # stage's background (it is short of F by a few 1e-9 for that reason alone); this one is as tight as the point's own
                # KKT residual.  One evaluation on all groups + one pricing launch.
                eps_c = float(prm.get("certificate_background", 1.0e-9))
                if ncap or eps_c <= 0.0:
                    break
                xs_n = np.maximum(xs, 0.0) / max(float(np.maximum(xs, 0.0).sum()), 1e-300)
                bufs.put("xs", xs_n)
                bufs.put("mu", mu)
                check(lib.bluest_support_point(L, S, sup_d.data_ptr(), bufs.ptr("xs"), cc.data_ptr(), eps_c, m_d.data_ptr(), st))
                evaluate(m_d, var_view)
                check(lib.bluest_price(plan._h, grad.data_ptr(), bufs.ptr("mu"), s_d.data_ptr(), cc.data_ptr(), S, sup_d.data_ptr(),
                                       bufs.ptr("csup"), bufs.ptr("topv"), bufs.ptr("topi"), bufs.ptr("y0"), st))
                h2 = bufs.fetch()
                if sharded is not None:
                    parts = gather((h2["topv"], h2["topi"], h2["csup"][:S]))
                    h2["topv"] = np.concatenate([p_[0] for p_ in parts])
                    h2["topi"] = np.concatenate([p_[1] for p_ in parts])
                    h2["csup"] = np.max(np.stack([p_[2] for p_ in parts]), axis=0)
                info["full_evals"] += 1
                A2 = 2.0 * float((mu / s) @ h2["y0"])
                cmax2 = max(float(h2["topv"].max()), float(h2["csup"][:S].max()))
                lb2 = A2 * A2 / (4.0 * cmax2) if (cmax2 > 0.0 and np.isfinite(A2)) else 0.0
                if np.isfinite(lb2) and lb2 > best_lb:
                    best_lb = lb2
                    cert = {"support": keep.copy(), "x": xs_n.copy(), "mu": mu.copy(), "background": eps_c, "lower_bound": lb2}
                if use_pre and not (np.isfinite(F_true) and 1.0 - best_lb / F_true <= 0.1 * stage_list[-1]):
                    info["pretrim_undone"] = info.get("pretrim_undone", 0) + 1
                    continue
                break
            stage_next = len(stage_list)
            if (not ncap and len(stage_list) == len(eps_list) and 0.0 < tight_eps < stage_list[-1] and np.isfinite(F_true)
                    and tight_gap < 1.0 - best_lb / F_true <= 0.1 * stage_list[-1]):
                # (a gap far above the last background is not the background's doing -- the ill-conditioned Navier-Stokes problem stops
                # at 1e-7 .. 1e-6 for its arithmetic, and a tighter stage only thrashes there: measured)
                stage_list.append(tight_eps)                      # from where the last stage ended (the polished point has lost the
                keep, xs, mu = stage_end                          # entries the tighter stage wants back: 8 more rounds instead of 3)
                info["tight_stage"] = True
                continue
            break
    lap("polish + final evaluations")
    if host_ms is not None:
        info["host_ms"] = {k_: round(v_, 3) for k_, v_ in host_ms.items()}
    if not np.isfinite(F_true):
        return None, "final allocation not evaluable"
    if 1.0 - best_lb / F_true > float(prm.get("give_up_gap", 1.0e-3)):
        # e.g. the optimal support does not fit the master's 64 entries: let the caller fall back rather than return this
        return None, "column generation ended with a certified gap of %.1e" % (1.0 - best_lb / F_true)
    x = np.zeros(L)
    x[keep] = np.maximum(xs, 0.0)
    x /= x.sum()
    if ncap:
        used = cap_system(keep, 0.0)[0] @ (np.maximum(xs, 0.0) / max(float(np.maximum(xs, 0.0).sum()), 1e-300))
        if (used > cap_rhs * (1.0 + 1.0e-9)).any():
            return None, "the final allocation violates a sample cap"
        info["cap_usage"] = used / cap_rhs
    info["t_rounds_ms"] = (_time.perf_counter() - _t_r0) * 1e3
    info.update({"F": F_true, "F_background": F_last, "lower_bound": best_lb, "gap": 1.0 - best_lb / F_true, "mu": mu,
                 "support": int((x > 0).sum()), "kkt": float(out[2]), "certificate": cert})
    return x, info

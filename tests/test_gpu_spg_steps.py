"""
Every launch of the device-resident SPG loop in isolation, and the loop in lock-step, against oracle/spg_device_ref.py.

A case uploads a crafted state and vectors, makes ONE C-ABI call and downloads everything the call may write (state, x, g, d,
xnew, m, enable; var / status / grad for the fused forms).  Then: words the reference calls untouched are bit-identical,
discrete words are equal, continuous words are within the reference's derived bound.  No bound here is measured; each is derived
in oracle/spg_device_ref.py next to its formula.

The tables (DECIDE_ROWS, DECIDE_FORMS, UPDATE_ROWS, UPDATE_KERNELS, PROJ_LENGTHS, LOCKSTEP) are data;
test_tables_cover_the_loop (CPU) fails when a projection instantiation, a decision form, an n_out class, an update kernel or a
row of the decision table is taken out.

Projection dispatch (csrc/spg.hip simplex_impl), which each length of PROJ_LENGTHS is meant for:
  no workspace or L <= 4096: k_simplex<4> L <= 2048 (64 / 128 / 256 / 512 threads for L <= 256 / 512 / 1024 / more),
      <12> <= 6144, <24> <= 12288, <48> <= 24576, <0> beyond
  workspace and L > 4096: k_proj_fused<ITEMS> with min(ceil(L / bt), CUs, 64) workgroups of bt = 256 (L <= 65536) or 1024
      threads, ITEMS = ceil(L / (bt * workgroups)) rounded up to 1, 2, 4, 8, 16; beyond 16 or under
      BLUEST_PROJ_MULTI_LAUNCH=1 the chain k_proj_a, k_proj_b<8> (L <= 8192) / k_proj_b<24> (L <= 24576) /
      k_proj_q0 + (k_proj_p, k_proj_q) x 5 + k_proj_b_finish, k_proj_c, k_proj_d
"""
import ctypes

import numpy as np
import pytest

from bluest_amd import synth
from oracle import spg_device_ref as ref

R = ref
INF = np.inf


# ---- which kernel a projection of length L gets -----------------------------------------------------------------------
def proj_kernel(L, cus, ws=True, multi=False):
    if ws and L > 4096:
        bt = 256 if L <= 64 * 256 * 4 else 1024
        nbf = max(1, min(-(-L // bt), cus, 64))
        items = -(-L // (bt * nbf))
        if items <= 16 and not multi:
            return ("fused", next(i for i in (1, 2, 4, 8, 16) if items <= i), bt, nbf)
        return ("multi", "b8" if L <= 8192 else ("b24" if L <= 24576 else "pq"))
    block = 512
    while block > 64 and (block // 2) * 4 >= L:
        block //= 2
    return ("simplex", next((i for i in (4, 12, 24, 48) if L <= 512 * i), 0), block)


# (L, workspace, multi-launch) -> the kernel it is meant for on a device with >= 64 compute units
PROJ_LENGTHS = [
    (1, True, False), (100, True, False), (400, True, False), (1000, True, False), (2048, True, False),    # k_simplex<4>: 64..512 threads
    (4096, True, False), (6000, False, False),                                                          # k_simplex<12>
    (12000, False, False), (24000, False, False), (30000, False, False),                                # k_simplex<24>, <48>, <0>
    (5000, True, False), (21699, True, False), (40000, True, False),                                    # k_proj_fused<1,2,4> x 256
    (70000, True, False), (200000, True, False), (300000, True, False), (600000, True, False),          # k_proj_fused<2,4,8,16> x 1024
    (5000, True, True), (21699, True, True), (30000, True, True),                                       # k_proj_b<8>, <24>, q0/p/q/finish
]
PROJ_REQUIRED = ({("simplex", i, 512) for i in (4, 12, 24, 48, 0)} | {("simplex", 4, b) for b in (64, 128, 256)}
                 | {("multi", k) for k in ("b8", "b24", "pq")})
# with at least 64 compute units these (ITEMS, threads) pairs exist; <8> and <16> never run with 256 threads and <1> never with 1024
PROJ_FUSED_64CU = {(1, 256), (2, 256), (4, 256), (2, 1024), (4, 1024), (8, 1024), (16, 1024)}

# ---- decision table ---------------------------------------------------------------------------------------------------
# row -> overrides of the base state / inputs: F_rel = objective of the trial relative to 1 (the base history maximum),
# words = state words, status / nan = output 1's status / V, expect = (accept, what else)
DECIDE_ROWS = {
    "accept": dict(F=0.9),
    "armijo_slope": dict(F=0.95, words={R.GD: -100.0}),          # between fmax + 1e-3 a gd and fmax + 1e-4 a gd: accepted
    "reject_small_alpha": dict(F=1.2, words={R.ALPHA: 0.05}),
    "reject_interp_inside": dict(F=1.2),                          # at = 0.25 / 0.7
    "reject_interp_upper_part": dict(F=0.857, words={R.HIST: 0.5}),   # at = 0.70 in (0.5 a, 0.9 a]
    "reject_interp_below": dict(F=5.0),                           # at = 0.055 < 0.1 -> a / 2
    "reject_interp_above": dict(F=0.75, words={R.HIST: 0.5}),     # at = 1.0 > 0.9 a -> a / 2
    "status_inf": dict(F=0.9, status=1),                          # max|m| < 0.05
    "status_no_model0": dict(F=0.9, status=2),
    "status_singular": dict(F=0.9, status=3),
    "nan_variance": dict(F=0.9, nan=True),
    "not_last_slot": dict(F=1.2, last=0),
    "accept_not_last_slot": dict(F=0.9, last=0),
    "alpha_underflow_fails": dict(F=1.2, words={R.ALPHA: 1.5e-300}),
    "maxfev_fails": dict(F=1.2, words={R.COUNT: 9.0, R.MAXFEV: 10.0}),
    "accept_already_set": dict(F=1.2, words={R.ACCEPT: 1.0}),
    "done_set": dict(F=0.9, words={R.DONE: 1.0}),
    "fail_set": dict(F=0.9, words={R.FAIL: 1.0}),
    "done_and_accept_set": dict(F=0.9, words={R.DONE: 1.0, R.ACCEPT: 1.0}),
    "pending_cleared_on_accept": dict(F=0.9, words={R.PENDING: 1.0}),
    "p32": dict(F=0.9, p=32.0), "p32_reject": dict(F=1.2, p=32.0),
    "p2048": dict(F=0.9, p=2048.0), "p2048_reject": dict(F=1.2, p=2048.0),
    "tie_at_the_maximum": dict(F=0.9, tie=True), "tie_p32": dict(F=0.9, tie=True, p=32.0),
    "hlen1": dict(F=0.9, H=1), "hlen1_reject": dict(F=1.2, H=1),
    "hlen16_max_in_last_slot": dict(F=0.9, H=16), "hlen16_reject": dict(F=1.2, H=16),
    "hlen10_max_in_last_slot": dict(F=0.9, H=10),
}
# spelled out, so that deleting a row from the table fails the guard
DECIDE_REQUIRED_ROWS = {
    "accept", "armijo_slope", "reject_small_alpha", "reject_interp_inside", "reject_interp_upper_part", "reject_interp_below",
    "reject_interp_above", "status_inf", "status_no_model0", "status_singular", "nan_variance", "not_last_slot",
    "accept_not_last_slot", "alpha_underflow_fails", "maxfev_fails", "accept_already_set", "done_set", "fail_set",
    "done_and_accept_set", "pending_cleared_on_accept", "p32", "p32_reject", "p2048", "p2048_reject", "tie_at_the_maximum",
    "tie_p32", "hlen1", "hlen1_reject", "hlen16_max_in_last_slot", "hlen16_reject", "hlen10_max_in_last_slot"}
# form -> (plan shape or None, n_out values)
DECIDE_FORMS = {
    "spg_decide": (None, (1, 2, 3, 8, 64)),
    "eval_decide": ("small", (1, 2, 3, 8)),
    "eval_grad_decide": ("large", (1, 2, 3, 8)),
    "solve_grad": ("large", (1, 2, 3, 8)),
}
FUSED_FORMS = [(f, o) for f in DECIDE_FORMS if f != "spg_decide" for o in DECIDE_FORMS[f][1]]
# plan shapes.  small / large: synth.problem(n, kmax), every output on all groups (identity plans), L = 175 (a small plan) and
# L = 21699 (> 4096).  ragged6: the ragged MOSAP of tests/golden/mosap_n6_o3_ragged.npz (3 outputs, 40 groups, mapped).
# mapped_large: the 21699 groups of n = 20, k <= 5, every output keeping the singletons and a random 70 % of the rest (mapped,
# > 5000 groups each).  k8 / k12 / k14: singletons, all pairs and 30 random groups of the widest size: small plans whose finish
# is k_spg_finish_small<8>, <12> and the generic tile.
PLAN_SHAPES = {"small": (10, 3), "large": (20, 5), "ragged6": (6, 3), "mapped_large": (20, 5), "k8": (12, 8), "k12": (14, 12), "k14": (16, 14)}

# ---- update table -------------------------------------------------------------------------------------------------------
UPDATE_ROWS = {
    "ratio_inside": dict(),
    "ratio_below_lmin": dict(words={R.LMIN: 1e6}),
    "ratio_above_lmax": dict(words={R.LMAX: 1e-9}),
    "sdoty_negative": dict(flip_y=True),
    "floor_1e-8": dict(floor=1e-8),
    "floor_1e-8_sdoty_negative": dict(floor=1e-8, flip_y=True),
    "ring_wraps": dict(words={R.IT: 9.0}),                    # IT + 1 = 10 = HLEN -> slot 0
    "ring_wraps_hlen16": dict(words={R.IT: 31.0, R.HLEN: 16.0}),
    "accept_clear": dict(words={R.ACCEPT: 0.0}),
    "done_set": dict(words={R.DONE: 1.0}),
    "fail_set": dict(words={R.FAIL: 1.0}),
}
UPDATE_LENGTHS = (1, 1023, 1024, 1025, 21699, 600000)        # 600000 > 512 x 1024: the grid-stride loop under the block cap
# update kernel -> the (entry point, plan shape, n_out) cases that run it; test_update_fused_and_finish is parametrised by this table
UPDATE_KERNELS = {
    "k_spg_update_a": [("update", None, 1)],                                        # test_update_table, at UPDATE_LENGTHS
    "k_spg_update_a_fused/identity": [("fused", "large", 1), ("fused", "large", 3), ("fused", "large", 8)],
    "k_spg_update_a_fused/mapped": [("fused", "ragged6", 3), ("fused", "mapped_large", 1), ("fused", "mapped_large", 3)],
    "k_spg_finish_small<5>": [("finish", "small", 1), ("finish", "small", 3), ("finish", "small", 8), ("finish", "ragged6", 3)],
    "k_spg_finish_small<8>": [("finish", "k8", 1), ("finish", "k8", 3)],
    "k_spg_finish_small<12>": [("finish", "k12", 1), ("finish", "k12", 3)],
    "k_spg_finish_small/generic tile": [("finish", "k14", 1), ("finish", "k14", 3)],
}
UPDATE_REQUIRED = {"k_spg_update_a", "k_spg_update_a_fused/identity", "k_spg_update_a_fused/mapped", "k_spg_finish_small<5>",
                   "k_spg_finish_small<8>", "k_spg_finish_small<12>", "k_spg_finish_small/generic tile"}
PLAN_UPDATE_CASES = [(k,) + c for k, cases in UPDATE_KERNELS.items() for c in cases if c[1] is not None]
FINISH_KMAX = {"k_spg_finish_small<5>": (1, 5), "k_spg_finish_small<8>": (6, 8), "k_spg_finish_small<12>": (9, 12),
               "k_spg_finish_small/generic tile": (13, 32)}
# ---- lock-step runs: name -> (plan shape, n_out, p, floor, slots, sequence, special) -------------------------------------
LOCKSTEP = {
    "small_o1": ("small", 1, INF, 0.0, 1, "window", None),
    "small_o3_p32_slots3": ("small", 3, 32.0, 0.0, 3, "window", None),
    "small_o3_floor_slots2": ("small", 3, INF, 1e-8, 2, "window", None),
    "n20_k5_o1": ("large", 1, INF, 0.0, 1, "window", None),
    "n20_k5_o8_p32_floor_slots2": ("large", 8, 32.0, 1e-8, 2, "window", None),
    "n20_k5_o1_sharded_sequence": ("large", 1, INF, 0.0, 1, "sharded", None),
    "mapped_o3_p32_floor_slots2": ("mapped_large", 3, 32.0, 1e-8, 2, "window", None),
    "small_o1_maxfev_ends_in_fail": ("small", 1, INF, 0.0, 1, "window", "fail"),
    "n20_k5_o1_eps_ends_in_done": ("large", 1, INF, 0.0, 1, "window", "done"),
}
LOCKSTEP_ITERATIONS = 60
UNDECIDABLE_CAP = 1.0 / 20.0          # tests/test_spg_device_ref.py holds the restatement itself to the same cap


def test_tables_cover_the_loop():
    """CPU: the tables above reach every projection kernel, decision form, n_out class, update kernel and decision row"""
    seen = {proj_kernel(L, 256, ws, multi) for L, ws, multi in PROJ_LENGTHS}
    assert PROJ_REQUIRED <= {k[:3] if k[0] == "simplex" else k for k in seen}, PROJ_REQUIRED - seen
    assert {(k[1], k[2]) for k in seen if k[0] == "fused"} == PROJ_FUSED_64CU
    assert set(DECIDE_FORMS) == {"spg_decide", "eval_decide", "eval_grad_decide", "solve_grad"}
    for form, (shape, n_outs) in DECIDE_FORMS.items():
        assert 1 in n_outs and any(o > 1 for o in n_outs), form             # the register tail and the last-arriver tail
    assert 64 in DECIDE_FORMS["spg_decide"][1] and {1, 2, 3, 8} <= set(DECIDE_FORMS["eval_grad_decide"][1])
    assert set(DECIDE_ROWS) == DECIDE_REQUIRED_ROWS
    assert set(UPDATE_KERNELS) == UPDATE_REQUIRED and all(UPDATE_KERNELS[k] for k in UPDATE_KERNELS)
    for k, cases in UPDATE_KERNELS.items():
        assert {c[2] == 1 for c in cases} == {True, False} or k in ("k_spg_update_a", "k_spg_update_a_fused/mapped"), k
        for entry, shape, n_out in cases:
            if k in FINISH_KMAX:
                assert entry == "finish" and FINISH_KMAX[k][0] <= PLAN_SHAPES[shape][1] <= FINISH_KMAX[k][1], (k, shape)
    assert {c[1] for c in UPDATE_KERNELS["k_spg_update_a_fused/mapped"]} == {"ragged6", "mapped_large"}
    assert {f for f, _ in FUSED_FORMS} == set(DECIDE_FORMS) - {"spg_decide"}
    for f in ("eval_decide", "eval_grad_decide", "solve_grad"):
        assert {1, 2, 3, 8} <= set(DECIDE_FORMS[f][1]), f
    assert {"sdoty_negative", "ring_wraps", "accept_clear", "done_set", "fail_set", "ratio_below_lmin", "ratio_above_lmax",
            "floor_1e-8"} <= set(UPDATE_ROWS)
    assert set(UPDATE_LENGTHS) >= {1, 1023, 1024, 1025, 21699, 600000}
    shapes = {(v[0], v[1] > 1) for v in LOCKSTEP.values()}
    assert shapes == {("small", False), ("small", True), ("large", False), ("large", True), ("mapped_large", True)}
    assert {v[4] for v in LOCKSTEP.values()} == {1, 2, 3} and {v[5] for v in LOCKSTEP.values()} == {"window", "sharded"}
    assert {v[6] for v in LOCKSTEP.values()} == {None, "fail", "done"}
    assert {v[2] for v in LOCKSTEP.values()} == {32.0, INF} and {v[3] for v in LOCKSTEP.values()} == {0.0, 1e-8}


# ---- rig ----------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def gpu():
    import torch
    assert torch.cuda.is_available(), "these tests need the MI355X"
    return torch


_PLANS = {}


def _plan(shape, n_out):
    """(Plan, scale, maps): maps[o] = global index of every local group of output o"""
    from bluest_amd.plan import Plan
    from conftest import golden
    key = (shape, n_out)
    if key in _PLANS:
        return _PLANS[key]
    n, kmax = PLAN_SHAPES[shape]
    rng = np.random.RandomState(n * 100 + kmax)
    if shape in ("small", "large"):
        prob = synth.problem(n, kmax, n_out)
        G = [np.asarray(g, dtype=np.int64).reshape(-1, k) for k, g in enumerate(prob["groups"], start=1)]
        scale = prob["budget"] / prob["costs"]
        local = [G] * n_out
    elif shape == "ragged6":
        gold = golden("mosap_n6_o3_ragged.npz")
        assert n_out == int(gold["n_out"])
        G = [gold["g_k%d" % k] for k in range(1, kmax + 1)]
        local = [[gold["mg%d_k%d" % (o, k)] for k in range(1, kmax + 1)] for o in range(n_out)]
        scale = None
    else:
        if shape == "mapped_large":
            G = [np.asarray(g, dtype=np.int64).reshape(-1, k) for k, g in enumerate(synth.all_groups(n, kmax), start=1)]
            local = [[g if k == 1 else g[rng.rand(len(g)) < 0.7] for k, g in enumerate(G, start=1)] for _ in range(n_out)]
        else:
            wide = sorted({tuple(sorted(rng.choice(n, kmax, replace=False).tolist())) for _ in range(30)})
            G = [np.arange(n).reshape(-1, 1), synth.all_groups(n, 2)[1]]
            G += [np.zeros((0, k), dtype=np.int64) for k in range(3, kmax)] + [np.array(wide, dtype=np.int64)]
            G = [np.asarray(g, dtype=np.int64).reshape(-1, k) for k, g in enumerate(G, start=1)]
            local = [G] * n_out
        scale = None
    L = sum(len(g) for g in G)
    flat = {tuple(int(x) for x in g): i for i, g in enumerate(g for gk in G for g in gk)}
    identity = all(lg is G for lg in local)
    maps = [np.arange(L) if identity else np.array([flat[tuple(int(x) for x in g)] for gk in lg for g in gk], dtype=np.int64) for lg in local]
    if scale is None:
        scale = L * (0.5 + rng.rand(L))                          # m = scale * x of order 1 for x on the simplex
    C = [synth.wishart_covariance(n, o)[0] for o in range(n_out)] if shape not in ("small", "large") else prob["C"]
    outs = [{"K": kmax, "sizes": [len(g) for g in local[o]], "groups": local[o], "C": C[o], "mapping": None if identity else maps[o]}
            for o in range(n_out)]
    plan = Plan(n, L, outs)
    assert plan.identity == identity and plan.launch_config(1)["kmax"] == kmax
    if shape == "mapped_large":
        assert min(len(mp) for mp in maps) >= 5000
    _PLANS[key] = (plan, scale, maps)
    return _PLANS[key]


class Rig(object):
    """the buffers of one device SPG loop, with poison in everything a launch is not supposed to touch"""
    VECS = ("x", "g", "d", "xnew", "m")

    def __init__(self, torch, L, n_out=1, plan=None, ws=True):
        from bluest_amd import _lib
        from bluest_amd.plan import projection_workspace, _stream
        self.torch, self.L, self.n_out, self.plan = torch, L, n_out, plan
        self.lib = _lib.lib()
        self.check, self.stream = _lib.check, _stream
        self.dev = plan.device if plan is not None else torch.device("cuda", torch.cuda.current_device())
        rng = np.random.RandomState(L % 9973 + n_out)
        up = lambda a: torch.from_numpy(np.ascontiguousarray(a)).to(self.dev)       # noqa: E731
        self.t = {k: up(rng.rand(L) + 2.0) for k in self.VECS}
        self.t["gnew"] = up(rng.rand(L) + 2.0)
        self.t["scale"] = up(0.5 + rng.rand(L))
        self.t["st"] = up(np.zeros(R.STATE_DOUBLES))
        self.t["var"] = up(np.full(max(n_out, 1), 7.25))
        self.t["status"] = up(np.full(max(n_out, 1), 77, dtype=np.int32))
        self.t["enable"] = up(np.full(1, 5, dtype=np.int32))
        self.t["work"] = up(np.zeros(1024))
        glen = plan.grad_len if plan is not None else 1
        self.t["grad"] = up(np.full(glen, 7.25))
        self.t["rec"] = up(np.zeros(n_out * plan.reclen)) if plan is not None else None
        self.pws = projection_workspace(L, self.dev) if ws else None
        if plan is not None:
            v = ctypes.c_void_p()
            self.check(self.lib.bluest_plan_v_workspace(plan._h, ctypes.byref(v), None))
            self.v_ws = v.value

    def p(self, name):
        return self.t[name].data_ptr()

    def put(self, **arrays):
        for k, a in arrays.items():
            self.t[k].copy_(self.torch.from_numpy(np.ascontiguousarray(a, dtype=np.int32 if k in ("status", "enable") else np.float64)))

    def snap(self):
        self.torch.cuda.synchronize()
        out = {k: self.t[k].cpu().numpy().copy() for k in self.VECS + ("st", "var", "status", "enable", "grad", "gnew")}
        if self.pws is not None and self.L > 4096:
            off = 2 * self.L + 4 * max((self.L + 1023) // 1024, 64)                 # ProjWs::tau_off
            t12 = float(self.pws[off + 12])
            assert t12 == 0.0, "the single-launch projection reported a timed-out wait"
        return out

    def gd_parts(self, n):
        return self.pws[2 * self.L:2 * self.L + 4 * n].cpu().numpy().reshape(n, 4)[:, 1].copy()

    def gate(self, on):
        self.check(self.lib.bluest_plan_set_gate(self.plan._h, self.p("enable") if on else None, 1 if on else 0))

    # -- launches
    def direction(self, z=1.0, floor=0.0):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_spg_direction(self.p("x"), self.p("g"), self.p("st"), z, floor, self.L, self.p("d"), self.p("scale"),
                                                     self.p("xnew"), self.p("m"), self.p("enable"),
                                                     None if self.pws is None else self.pws.data_ptr(), self.stream()))

    def converged(self, z=1.0, floor=0.0):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_spg_converged(self.p("x"), self.p("g"), self.p("st"), z, floor, self.L,
                                                     None if self.pws is None else self.pws.data_ptr(), self.stream()))

    def trial(self):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_spg_trial(self.p("x"), self.p("d"), self.p("scale"), self.p("st"), self.p("xnew"), self.p("m"),
                                                 self.p("enable"), self.L, self.stream()))

    def decide(self, form, last):
        lib, h = self.lib, (self.plan._h if self.plan is not None else None)
        with self.torch.cuda.device(self.dev):
            if form == "spg_decide":
                self.check(lib.bluest_spg_decide(self.p("st"), self.p("var"), self.p("status"), self.n_out, last, self.p("enable"), self.stream()))
            elif form == "eval_decide":
                self.check(lib.bluest_plan_eval_decide(h, self.p("m"), 0.0, self.p("var"), self.p("status"), self.p("st"), last,
                                                       self.p("enable"), self.stream()))
            elif form == "eval_grad_decide":
                self.check(lib.bluest_plan_eval_grad_decide(h, self.p("m"), 0.0, self.p("var"), self.p("grad"), self.p("status"), self.p("st"),
                                                            last, self.p("enable"), self.stream()))
            else:
                self.check(lib.bluest_plan_phi(h, self.p("m"), 1, self.L, self.p("rec"), self.stream()))
                self.check(lib.bluest_plan_solve_grad(h, self.p("rec"), 0.0, self.p("var"), self.p("grad"), self.p("status"), self.p("st"), last,
                                                      self.p("enable"), self.stream()))

    def update(self, floor=0.0):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_spg_update(self.p("x"), self.p("g"), self.p("xnew"), self.p("gnew"), self.p("st"), floor, self.L,
                                                  self.p("work"), self.stream()))

    def update_fused(self, floor=0.0):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_spg_update_fused(self.plan._h, self.p("x"), self.p("g"), self.p("xnew"), self.p("grad"), self.p("scale"),
                                                        self.p("st"), floor, self.p("work"), self.stream()))

    def finish(self, floor=0.0):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_spg_finish(self.plan._h, self.v_ws, self.p("status"), self.p("x"), self.p("g"), self.p("xnew"),
                                                  self.p("grad"), self.p("scale"), self.p("st"), floor, self.p("work"), self.stream()))

    def combine(self):
        with self.torch.cuda.device(self.dev):
            self.check(self.lib.bluest_plan_combine_grad(self.plan._h, self.p("grad"), self.plan.grad_len, self.p("st") + 8 * R.COEF, self.p("scale"),
                                                         1, self.p("gnew"), self.L, self.stream()))


def bits(a):
    return np.ascontiguousarray(a).view(np.uint64 if a.dtype == np.float64 else np.uint32)


def check_launch(tag, before, after, la, scratch=(), frozen=("var", "status", "grad", "gnew")):
    """after = before except where the reference launch `la` writes; there: equal (bound 0) or within the bound"""
    sb, sa = before["st"], after["st"]
    for w in range(R.STATE_DOUBLES):
        if w in scratch:
            continue
        if not la.written[w]:
            assert bits(sb[w:w + 1])[0] == bits(sa[w:w + 1])[0], (tag, "state word %d changed: %r -> %r" % (w, sb[w], sa[w]))
        elif la.bound[w] == 0.0:
            rng = la.extra.get("npos_range") if w in (R.NPOS, R.GPSTATS + 3) else None
            if rng:                                # entries within the bound of the threshold may count either way
                assert rng[0] <= sa[w] <= rng[1], (tag, "count", sa[w], rng)
            else:
                assert sa[w] == la.state[w], (tag, "state word %d: %r, expected %r" % (w, sa[w], la.state[w]))
        elif np.isfinite(la.bound[w]):
            assert abs(sa[w] - la.state[w]) <= la.bound[w], (tag, "state word %d: %r, expected %r +- %r" % (w, sa[w], la.state[w], la.bound[w]))
    for name in Rig.VECS:
        if name in la.vec:
            b = la.vbound[name]
            if np.isscalar(b) and b == 0.0:
                assert np.array_equal(bits(after[name]), bits(la.vec[name])), (tag, name, "not bit for bit")
            else:
                err = np.abs(after[name] - la.vec[name])
                i = int(np.argmax(err - b))
                assert (err <= b).all(), (tag, name, i, after[name][i], la.vec[name][i], np.broadcast_to(b, err.shape)[i])
        else:
            assert np.array_equal(bits(before[name]), bits(after[name])), (tag, name, "written by a launch that must not")
    if la.enable is None:
        assert after["enable"][0] == before["enable"][0], (tag, "enable changed")
    else:
        assert after["enable"][0] == la.enable, (tag, "enable", after["enable"][0], la.enable)
    for name in frozen:
        assert np.array_equal(bits(before[name]), bits(after[name])), (tag, name, "written by a launch that must not")


def base_state(n_out, H=10, p=INF):
    st = np.zeros(R.STATE_DOUBLES)
    st[R.F], st[R.ALPHA], st[R.GD], st[R.LAMBDA] = 1.0, 1.0, -0.5, 0.37
    st[R.NORM], st[R.P], st[R.LMIN], st[R.LMAX], st[R.HLEN] = 1.7, p, 1e-30, 1e3, H
    st[R.IT], st[R.COUNT], st[R.MAXFEV], st[R.EPS_W] = 3.0, 5.0, 1000.0, 1e-9
    st[R.HIST:R.HIST + 16] = -INF
    st[R.HIST:R.HIST + H] = 0.2
    st[R.HIST + H - 1] = 1.0                                        # the maximum sits in the LAST slot in use
    st[R.S:R.S + n_out] = 1.0 + 0.1 * np.arange(n_out)
    st[R.FNEW], st[R.FTRIAL], st[R.SDOTS], st[R.SDOTY] = 0.77, 0.66, 0.55, 0.44      # recognisable leftovers
    st[R.COEF:R.COEF + 64] = 0.125
    st[R.GPSTATS:R.GPSTATS + 4] = (0.1, 0.2, 0.3, 4.0)
    return st


def _row_state(row, n_out, ratios, var):
    """state for a decision row given the plan's (or crafted) V: S and NORM are set so that F comes out as row["F"] relative to
    the history maximum 1 (0.5 where the row lowers HIST) -- at least 1e-3 away from the Armijo threshold in every row"""
    H = row.get("H", 10)
    st = base_state(n_out, H, row.get("p", INF))
    if R.HIST in row.get("words", {}):
        st[R.HIST:R.HIST + H] = 0.2
        st[R.HIST + H - 1] = 0.5
    for w, v in row.get("words", {}).items():
        if w != R.HIST:
            st[w] = v
    st[R.S:R.S + n_out] = var / ratios                                # V_o / s_o = ratios_o
    probe = st.copy()
    probe[R.NORM] = 1.0
    F1 = R.objective(probe, var, np.zeros(n_out, dtype=np.int32), n_out)[0]
    st[R.NORM] = F1 / row["F"]
    return st


def _ratios(row, n_out):
    r = 1.0 - 0.013 * np.arange(n_out)
    if row.get("tie") and n_out > 2:
        r[1] = r[2] = 1.0
        r[0] = 0.9                                                     # outputs 1 and 2 tie at the maximum: 1 wins
    elif row.get("tie") and n_out == 2:
        r[:] = 1.0
    return r


def _check_decision(tag, rig, form, row, st, before, n_out, gd_parts=None):
    last = row.get("last", 1)
    rig.decide(form, last)
    after = rig.snap()
    la = R.decide(st, after["var"], after["status"], n_out, last, gd_parts=gd_parts)
    if not la.extra["early"]:
        assert la.extra["margin"] > 1e-3 * abs(la.extra["threshold"]) or not np.isfinite(la.extra["F"]), (tag, la.extra)
    frozen = ("gnew",) if form != "spg_decide" else ("var", "status", "grad", "gnew")
    check_launch(tag, before, after, la, frozen=frozen)
    return after, la


# ---- the decision table ---------------------------------------------------------------------------------------------------
@pytest.mark.gpu
@pytest.mark.parametrize("n_out", DECIDE_FORMS["spg_decide"][1])
def test_decide_table_standalone(gpu, n_out):
    rig = Rig(gpu, 64, n_out)
    for name, row in DECIDE_ROWS.items():
        ratios = _ratios(row, n_out)
        var = 0.003 * (1.0 + 0.5 * np.arange(n_out))
        st = _row_state(row, n_out, ratios, var)
        status = np.zeros(n_out, dtype=np.int32)
        bad = min(1, n_out - 1)
        if "status" in row:
            status[bad] = row["status"]
        if row.get("nan"):
            var = var.copy()
            var[bad] = np.nan
        rig.put(st=st, var=var, status=status, enable=np.full(1, 5, dtype=np.int32))
        before = rig.snap()
        after, la = _check_decision(("spg_decide", n_out, name), rig, "spg_decide", row, st, before, n_out)
        if "status" in row or row.get("nan"):
            assert after["st"][R.FTRIAL] == INF and after["st"][R.ACCEPT] == 0.0 and after["st"][R.ALPHA] == 0.5


@pytest.mark.gpu
@pytest.mark.parametrize("form,n_out", FUSED_FORMS)
def test_decide_table_fused(gpu, form, n_out):
    """the decision in the tail of the solve kernels: V comes from the plan, the state is set around it.  Every row is issued
    twice in a row on the same plan (a ticket left non-zero by the first call would keep the second from deciding)."""
    torch = gpu
    plan, scale, _ = _plan(DECIDE_FORMS[form][0], n_out)
    L = plan.L
    rig = Rig(torch, L, n_out, plan)
    rng = np.random.RandomState(3)
    x = (0.5 + rng.rand(L)) / L
    has0 = np.concatenate([(np.asarray(g) == 0).any(axis=1) for g in synth.problem(*PLAN_SHAPES[DECIDE_FORMS[form][0]], n_out)["groups"]])
    allocations = {"ok": scale * x, "status_inf": np.full(L, 0.01), "status_no_model0": scale * x * ~has0, "status_singular": -scale * x}
    var_ok, grad_ok, st_ok = plan.eval(allocations["ok"])
    var_ok = var_ok[0].cpu().numpy()
    assert (st_ok[0].cpu().numpy() == 0).all()
    rig.gate(True)
    try:
        for name, row in DECIDE_ROWS.items():
            if row.get("nan"):
                continue                                  # a NaN variance with status OK cannot come out of a plan
            m = allocations.get(name, allocations["ok"])
            st = _row_state(row, n_out, _ratios(row, n_out), var_ok)
            for rep in range(2):
                rig.put(st=st, m=m, enable=np.ones(1, dtype=np.int32), var=np.full(n_out, 7.25), status=np.full(n_out, 77, dtype=np.int32),
                        grad=np.full(plan.grad_len, 7.25))
                before = rig.snap()
                tag = (form, n_out, name, rep)
                after, la = _check_decision(tag, rig, form, row, st, before, n_out)
                if name.startswith("status_"):
                    want = {"status_inf": 1, "status_no_model0": 2, "status_singular": 3}[name]
                    assert (after["status"] == want).all(), (tag, after["status"])
                    assert after["st"][R.FTRIAL] == INF and after["st"][R.ACCEPT] == 0.0 and after["st"][R.ALPHA] == 0.5, tag
                if form == "eval_grad_decide" and name in ("accept", "reject_interp_inside"):
                    # same kernel, same summation order as bluest_plan_eval: bit for bit
                    rig.gate(False)
                    v2, g2, s2 = plan.eval(m)
                    rig.gate(True)
                    assert np.array_equal(bits(g2[0].cpu().numpy()), bits(after["grad"])), tag
                    assert np.array_equal(bits(v2[0].cpu().numpy()), bits(after["var"])), tag
        # the gate closed (an earlier slot accepted): nothing changes but the gate of the finishing launches.  As in the loop,
        # the slot before evaluated the same m with the gate open: the decision reopens the gate while the launch is running, and
        # a gradient workgroup that starts after that recomputes the same bits from the same Phi partials.  V, status and the
        # decision ticket belong to workgroups that must all have seen the gate closed: here they hold poison, and four calls
        # in a row must each leave it alone (regression: workgroup 0 used to decide at once, the others then saw the gate open,
        # solved from stale partials and left the ticket of the next decision non-zero).
        st = _row_state(DECIDE_ROWS["accept_already_set"], n_out, _ratios({}, n_out), var_ok)
        rig.put(st=st, m=allocations["ok"], enable=np.ones(1, dtype=np.int32))
        rig.decide(form, 0)
        for rep in range(4):
            rig.put(st=st, enable=np.zeros(1, dtype=np.int32), var=np.full(n_out, 7.25), status=np.full(n_out, 77, dtype=np.int32))
            before = rig.snap()
            rig.decide(form, 1)
            after = rig.snap()
            la = R.decide(st, before["var"], before["status"], n_out, 1)
            check_launch((form, n_out, "gate closed", rep), before, after, la)
            assert after["enable"][0] == 1
        # ... and the next open decision still waits for every output (a ticket left over would let it decide early)
        row = DECIDE_ROWS["reject_interp_inside"]
        st = _row_state(row, n_out, _ratios(row, n_out), var_ok)
        rig.put(st=st, enable=np.ones(1, dtype=np.int32), var=np.full(n_out, 7.25), status=np.full(n_out, 77, dtype=np.int32))
        before = rig.snap()
        _check_decision((form, n_out, "open after closed"), rig, form, row, st, before, n_out)
        if L > 4096:
            # GDPARTS_N > 0, left by a real multi-workgroup bluest_spg_direction on this state: the decision folds the partials
            # and ignores the (poisoned) GD word; the same case with GDPARTS_N = 0 and the folded value in GD decides alike
            ones = np.ones(1, dtype=np.int32)
            stq = base_state(n_out)
            rig.put(st=stq, x=np.ones(L) / L, g=rng.randn(L) * 3.0 / L, enable=ones)
            rig.direction(1.0, 0.0)
            dev = rig.snap()["st"]
            n_parts = int(dev[R.GDPARTS_N])
            assert n_parts > 1
            parts = rig.gd_parts(n_parts)
            for name in ("accept", "reject_interp_inside", "reject_small_alpha", "p32_reject"):
                row, got = DECIDE_ROWS[name], []
                for with_parts in (True, False):
                    st = _row_state(row, n_out, _ratios(row, n_out), var_ok)
                    st[R.GDPARTS] = dev[R.GDPARTS]
                    st[R.GDPARTS_N], st[R.GD] = (n_parts, 1e6) if with_parts else (0.0, float(parts.sum()))
                    rig.put(st=st, m=allocations["ok"], enable=ones, var=np.full(n_out, 7.25), status=np.full(n_out, 77, dtype=np.int32))
                    before = rig.snap()
                    after, la = _check_decision((form, n_out, name, "partials" if with_parts else "folded"), rig, form, row, st, before, n_out,
                                                gd_parts=parts if with_parts else None)
                    got.append(after["st"])
                for w in (R.ACCEPT, R.PENDING, R.FAIL, R.COUNT):
                    assert got[0][w] == got[1][w], (form, n_out, name, w)
                assert abs(got[0][R.ALPHA] - got[1][R.ALPHA]) <= 1e-12 * got[1][R.ALPHA]      # g.d folded in two orders: 64 EPS
    finally:
        rig.gate(False)


# ---- the update table ---------------------------------------------------------------------------------------------------
def _update_inputs(L, row, rng):
    x = (0.5 + rng.rand(L)) / L
    x[rng.rand(L) < 0.3] = 1e-12                               # entries below the floor 1e-8, the rest above it
    xnew = np.maximum(x + 0.1 * rng.randn(L) / L, 0.0)
    g = rng.randn(L)
    s = xnew - x
    y = 0.5 * s * L + 1e-3 * rng.randn(L) / L                  # s.y > 0, well away from 0
    if row.get("flip_y"):
        y = -y
    return x, g, xnew, g + y


def _update_state(row):
    st = base_state(3)
    st[R.ACCEPT], st[R.FNEW] = 1.0, 0.8125
    for w, v in row.get("words", {}).items():
        st[w] = v
    return st


@pytest.mark.gpu
@pytest.mark.parametrize("L", UPDATE_LENGTHS)
def test_update_table(gpu, L):
    rig = Rig(gpu, L, 1, ws=False)
    rng = np.random.RandomState(L % 1000)
    for name, row in UPDATE_ROWS.items():
        x, g, xnew, gnew = _update_inputs(L, row, rng)
        st = _update_state(row)
        floor = row.get("floor", 0.0)
        for rep in range(2):                                   # back to back: the ticket must be back at 0
            rig.put(st=st, x=x, g=g, xnew=xnew, gnew=gnew)
            before = rig.snap()
            rig.update(floor)
            after = rig.snap()
            la = R.update(st, x, g, xnew, gnew, floor)
            check_launch(("update", L, name, rep), before, after, la)
            if la.written.any():
                assert la.extra["sdoty_sign_sure"], (L, name)
                assert after["st"][R.HIST + la.extra["hist_slot"]] == st[R.FNEW]
            assert bits(after["st"][R.TICKET:R.TICKET + 1])[0] == 0


@pytest.mark.gpu
@pytest.mark.parametrize("which,kernel,shape,n_out", PLAN_UPDATE_CASES, ids=["%s-%s-o%d" % (c[0], c[2], c[3]) for c in PLAN_UPDATE_CASES])
def test_update_fused_and_finish(gpu, which, kernel, shape, n_out):
    """gnew_j = scale_j sum_o COEF_o grad_o[local_o(j)] formed inside the update (k_spg_update_a_fused, identity and mapped plans)
    and inside k_spg_finish_small<KU> / its generic tile, whose gradient tiles are also compared with bluest_plan_grad's"""
    torch = gpu
    plan, scale, maps = _plan(shape, n_out)
    L = plan.L
    assert plan.identity == which.endswith("identity") or kernel == "finish"
    if kernel == "finish":
        assert L <= 4096 and FINISH_KMAX[which][0] <= plan.launch_config(1)["kmax"] <= FINISH_KMAX[which][1]
    rig = Rig(torch, L, n_out, plan)
    rng = np.random.RandomState(11 + n_out)
    for name, row in UPDATE_ROWS.items():
        x, g, xnew, _ = _update_inputs(L, row, rng)
        st = _update_state(row)
        st[R.COEF:R.COEF + n_out] = (1.0 + rng.rand(n_out)) * (-1.0 if row.get("flip_y") else 1.0)
        floor = row.get("floor", 0.0)
        # gradient of the trial point: bluest_plan_eval leaves v / status in the plan's workspace, which finish reads
        var, grad, status = plan.eval(scale * xnew)
        assert (status[0].cpu().numpy() == 0).all()
        gh = grad[0].cpu().numpy()
        for rep in range(2):
            rig.put(st=st, x=x, g=g, xnew=xnew, scale=scale, status=status[0].cpu().numpy(),
                    grad=gh if kernel == "fused" else np.full(plan.grad_len, 7.25))
            before = rig.snap()
            (rig.update_fused if kernel == "fused" else rig.finish)(floor)
            after = rig.snap()
            tag = (kernel, n_out, name, rep)
            live = st[R.ACCEPT] != 0.0 and not R.idle(st)
            if kernel == "finish" and live:
                assert np.array_equal(bits(after["grad"]), bits(gh)), (tag, "gradient tiles differ from bluest_plan_grad's")
            grads = [(after["grad"] if live else gh)[plan.grad_off[o]:plan.grad_off[o] + len(maps[o])] for o in range(n_out)]
            gnew, bg = R.combine(st, grads, maps, scale, L, n_out)
            la = R.update(st, x, g, xnew, gnew, floor, gnew_bound=bg)
            check_launch(tag, before, after, la, frozen=("var", "status", "gnew") + (("grad",) if kernel == "fused" or not live else ()))
            assert bits(after["st"][R.TICKET:R.TICKET + 1])[0] == 0


# ---- direction, convergence projection, trial point ----------------------------------------------------------------------
def _proj_inputs(L, rng):
    x = rng.rand(L) + 0.1
    x[rng.rand(L) < 0.4] = 0.0
    if not x.any():
        x[0] = 1.0
    x /= x.sum()
    x[(rng.rand(L) < 0.1) & (x > 0)] = 1e-12                   # below the floor 1e-8
    return x, rng.randn(L) / max(L, 1) * 3.0, rng.rand(L) + 2.0


@pytest.mark.gpu
@pytest.mark.parametrize("L,ws,multi", PROJ_LENGTHS, ids=["L%d%s%s" % (L, "" if ws else "_nows", "_multi" if multi else "") for L, ws, multi in PROJ_LENGTHS])
def test_direction_and_converged(gpu, monkeypatch, L, ws, multi):
    torch = gpu
    if multi:
        monkeypatch.setenv("BLUEST_PROJ_MULTI_LAUNCH", "1")
    else:
        monkeypatch.delenv("BLUEST_PROJ_MULTI_LAUNCH", raising=False)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kern = proj_kernel(L, cus, ws, multi)
    wg = kern[3] if kern[0] == "fused" else 0
    rig = Rig(torch, L, 1, ws=ws)
    rng = np.random.RandomState(L % 997)
    x, g, d0 = _proj_inputs(L, rng)
    scale = 0.5 + rng.rand(L)
    rig.put(scale=scale)
    lambdas = (0.37, 0.0, 1e-30, 1.0, 1e3, 1e-3)                # the last: a warm start from a very different lambda
    for floor in (0.0, 1e-8):
        for lam in lambdas:
            st = base_state(1)
            st[R.LAMBDA] = lam
            st[R.GD] = 1e6                                       # a multi-workgroup direction leaves this word alone
            rig.put(st=st, x=x, g=g, d=d0, enable=np.full(1, 5, dtype=np.int32))
            before = rig.snap()
            rig.direction(1.0, floor)
            after = rig.snap()
            la = R.direction(st, x, g, d0, scale, 1.0, floor, workgroups=wg)
            tag = ("direction", kern, floor, lam)
            check_launch(tag, before, after, la, scratch=R.SCRATCH)
            if wg:
                # the g.d the decision will use: per-workgroup partials, folded as the decision folds them
                parts = rig.gd_parts(wg)
                assert abs(parts.sum() - la.extra["gd"]) <= la.extra["gd_bound"] + wg * R.EPS * np.abs(parts).sum(), tag
                if lam == 0.37:
                    assert abs(la.extra["gd"]) > la.extra["gd_bound"], tag       # a slope whose sign is beyond its bound
                    # a following decision must take g.d from the partials, not from the stale GD word: a trial that the true
                    # slope rejects and the stale 1e6 would accept
                    st2 = after["st"].copy()
                    var = np.array([(1.0 + 1e-4 * la.extra["gd"] + 0.5e-4 * abs(la.extra["gd"])) * st2[R.NORM] * st2[R.S]])    # half a slope above the threshold 1 + 1e-4 g.d
                    ok1 = np.zeros(1, dtype=np.int32)
                    rig.put(var=var, status=ok1)
                    b2 = rig.snap()
                    rig.decide("spg_decide", 1)
                    a2 = rig.snap()
                    ld = R.decide(st2, var, ok1, 1, 1, gd_parts=parts)
                    assert ld.extra["margin"] > 0 and not ld.extra["accept"], (tag, ld.extra)
                    check_launch(tag + ("decide",), b2, a2, ld)
        # PENDING: the next trial point, bit for bit; d and the statistics untouched
        st = base_state(1)
        st[R.PENDING], st[R.ALPHA] = 1.0, 0.3173
        rig.put(st=st, x=x, g=g, d=d0, enable=np.full(1, 5, dtype=np.int32))
        before = rig.snap()
        rig.direction(1.0, floor)
        check_launch(("pending", kern, floor), before, rig.snap(), R.direction(st, x, g, d0, scale, 1.0, floor, workgroups=wg))
        for word in (R.DONE, R.FAIL):
            st = base_state(1)
            st[word] = 1.0
            rig.put(st=st, x=x, g=g, d=d0, enable=np.full(1, 5, dtype=np.int32))
            before = rig.snap()
            rig.direction(1.0, floor)
            check_launch(("idle direction", kern, word), before, rig.snap(), R.direction(st, x, g, d0, scale, 1.0, floor, workgroups=wg))
            before = rig.snap()
            rig.converged(1.0, floor)
            check_launch(("idle converged", kern, word), before, rig.snap(), R.converged(st, x, g, 1.0, floor))
        # convergence projection: EPS a factor 2 below and above the reference's max|gp|
        gpmax = R.converged(base_state(1), x, g, 1.0, floor).state[R.GPSTATS + 1]
        for factor, done in ((0.5, 0.0), (2.0, 1.0)):
            st = base_state(1)
            st[R.EPS_W] = factor * gpmax
            st[R.PENDING] = 1.0 if factor == 2.0 else 0.0         # PENDING does not concern this projection
            rig.put(st=st, x=x, g=g, d=d0, enable=np.full(1, 5, dtype=np.int32))
            before = rig.snap()
            rig.converged(1.0, floor)
            after = rig.snap()
            la = R.converged(st, x, g, 1.0, floor)
            assert la.extra["done_margin"] > 0
            check_launch(("converged", kern, floor, factor), before, after, la, scratch=R.SCRATCH)
            assert after["st"][R.DONE] == done


@pytest.mark.gpu
def test_projection_cases_reach_every_kernel_of_this_device(gpu):
    """which k_proj_fused<ITEMS> x workgroup size a length gets depends on the number of compute units: the set PROJ_LENGTHS
    reaches on THIS device must be every pair any length can get here (a scan over all lengths the single launch accepts)"""
    cus = gpu.cuda.get_device_properties(0).multi_processor_count
    seen = {proj_kernel(L, cus, ws, multi) for L, ws, multi in PROJ_LENGTHS}
    reachable = {proj_kernel(L, cus)[1:3] for L in list(range(4097, 70000, 61)) + list(range(65537, 64 * 1024 * 16 + 1, 509))
                 if proj_kernel(L, cus)[0] == "fused"}
    assert {k[1:3] for k in seen if k[0] == "fused"} == reachable, (cus, reachable)
    assert PROJ_REQUIRED <= seen


@pytest.mark.gpu
@pytest.mark.parametrize("L", [1, 1023, 1024, 1025, 5000])
def test_trial(gpu, L):
    rig = Rig(gpu, L, 1, ws=False)
    rng = np.random.RandomState(L)
    x, d, scale = rng.rand(L), rng.randn(L), 0.5 + rng.rand(L)
    rig.put(x=x, d=d, scale=scale)
    for words in ({}, {R.ALPHA: 0.3173}, {R.PENDING: 1.0}, {R.ACCEPT: 1.0}, {R.DONE: 1.0}, {R.FAIL: 1.0}):
        st = base_state(1)
        for w, v in words.items():
            st[w] = v
        rig.put(st=st, enable=np.full(1, 5, dtype=np.int32))
        before = rig.snap()
        rig.trial()
        check_launch(("trial", L, tuple(words)), before, rig.snap(), R.trial(st, x, d, scale))


# ---- lock-step -------------------------------------------------------------------------------------------------------------
def _start(rig, plan, scale, n_out, p, floor, maxfev=10 ** 6, eps=0.0, maps=None):
    """the state DeviceSpg.run uploads: uniform x, its gradient, F normalised to 1"""
    L = plan.L
    x = np.ones(L) / L
    var, grad, status = plan.eval(scale * x)
    var, grad = var[0].cpu().numpy(), grad[0].cpu().numpy()
    s_norm = np.ones(n_out)
    st0 = np.zeros(R.STATE_DOUBLES)
    st0[R.NORM], st0[R.P] = 1.0, p
    st0[R.S:R.S + n_out] = s_norm
    F0, _, coef, _ = R.objective(st0, var, status[0].cpu().numpy(), n_out)
    st0[R.COEF:R.COEF + n_out] = coef / F0
    maps = [np.arange(L)] * n_out if maps is None else maps
    grads = [grad[plan.grad_off[o]:plan.grad_off[o] + len(maps[o])] for o in range(n_out)]
    g = R.combine(st0, grads, maps, scale, L, n_out)[0]
    gpmax = R.project(x, g, 1.0, 1.0, floor)[4][1]
    st = R.initial_state(F0, gpmax, n_out, s_norm, p, 10, 1e-30, 1e3, eps if eps else 0.0, maxfev)
    rig.put(st=st, x=x, g=g, d=np.zeros(L), xnew=x, m=scale * x, scale=scale, enable=np.ones(1, dtype=np.int32),
            var=np.zeros(n_out), status=np.zeros(n_out, dtype=np.int32), grad=np.zeros(plan.grad_len))
    return gpmax


@pytest.mark.gpu
@pytest.mark.parametrize("name", sorted(LOCKSTEP))
def test_lockstep(gpu, name):
    """the launch sequence of bluest_spg_window (or of ShardedDeviceSpg._window_direct) call by call; after every call the
    reference launch, fed with the device's PREVIOUS snapshot (and, for the decision, the device's V / status / gradient of that
    slot), must agree within the single-launch bounds.  Rounding differences therefore cannot grow along the run."""
    torch = gpu
    shape, n_out, p, floor, slots, sequence, special = LOCKSTEP[name]
    plan, scale, maps = _plan(shape, n_out)
    L = plan.L
    small = shape == "small"
    rig = Rig(torch, L, n_out, plan)
    cus = torch.cuda.get_device_properties(0).multi_processor_count
    kern = proj_kernel(L, cus, True, False)
    wg = kern[3] if kern[0] == "fused" else 0
    _start(rig, plan, scale, n_out, p, floor, maxfev=6 if special == "fail" else 10 ** 6, maps=maps)
    form = "solve_grad" if sequence == "sharded" else ("eval_decide" if small else "eval_grad_decide")
    decisions = undecidable = 0
    saw_pending = saw_idle_launches = False
    rig.gate(True)
    try:
        cur = rig.snap()
        for it in range(LOCKSTEP_ITERATIONS):
            tag = (name, it)
            was_idle = R.idle(cur["st"])
            saw_pending = saw_pending or cur["st"][R.PENDING] == 1.0
            rig.direction(1.0, floor)
            nxt = rig.snap()
            la = R.direction(cur["st"], cur["x"], cur["g"], cur["d"], scale, 1.0, floor, workgroups=wg)
            check_launch(tag + ("direction",), cur, nxt, la, scratch=R.SCRATCH)
            cur = nxt
            for t in range(slots):
                last = 1 if t == slots - 1 else 0
                if t > 0:
                    rig.trial()
                    nxt = rig.snap()
                    check_launch(tag + ("trial", t), cur, nxt, R.trial(cur["st"], cur["x"], cur["d"], scale))
                    cur = nxt
                gate_open = cur["enable"][0] != 0
                rig.decide(form, last)
                nxt = rig.snap()
                parts = rig.gd_parts(int(cur["st"][R.GDPARTS_N])) if cur["st"][R.GDPARTS_N] > 0 else None
                la = R.decide(cur["st"], nxt["var"], nxt["status"], n_out, last, gd_parts=parts)
                if not la.extra["early"]:
                    decisions += 1
                    if not la.extra["margin"] > 0:
                        undecidable += 1
                        la = R.decide(cur["st"], nxt["var"], nxt["status"], n_out, last, gd_parts=parts, force_accept=nxt["st"][R.ACCEPT] != 0.0)
                    if "alpha_alt" in la.extra and abs(nxt["st"][R.ALPHA] - la.extra["alpha_alt"]) <= la.extra["alpha_alt_bound"]:
                        la.put(R.ALPHA, la.extra["alpha_alt"], la.extra["alpha_alt_bound"])      # the safeguard within its bound
                if not gate_open:
                    assert np.array_equal(bits(cur["var"]), bits(nxt["var"])) and np.array_equal(bits(cur["grad"]), bits(nxt["grad"])), tag
                check_launch(tag + ("decide", t), cur, nxt, la, frozen=("gnew",))
                cur = nxt
            live = cur["st"][R.ACCEPT] != 0.0 and not R.idle(cur["st"])
            if sequence == "sharded":
                rig.combine()
                rig.update(floor)
                nxt = rig.snap()
                if cur["enable"][0]:
                    # bluest_plan_combine_grad against the restated fold of the device's gradient, within its bound
                    grads = [cur["grad"][plan.grad_off[o]:plan.grad_off[o] + len(maps[o])] for o in range(n_out)]
                    gref, bg = R.combine(cur["st"], grads, maps, scale, L, n_out)
                    assert (np.abs(nxt["gnew"] - gref) <= bg).all(), tag + ("combine_grad",)
                else:
                    assert np.array_equal(bits(nxt["gnew"]), bits(cur["gnew"])), tag + ("combine_grad ran with the gate closed",)
                la = R.update(cur["st"], cur["x"], cur["g"], cur["xnew"], nxt["gnew"], floor)
                check_launch(tag + ("update",), cur, nxt, la, frozen=("var", "status", "grad"))
            else:
                (rig.finish if small else rig.update_fused)(floor)
                nxt = rig.snap()
                grads = [nxt["grad"][plan.grad_off[o]:plan.grad_off[o] + len(maps[o])] for o in range(n_out)]
                gnew, bg = R.combine(cur["st"], grads, maps, scale, L, n_out)
                la = R.update(cur["st"], cur["x"], cur["g"], cur["xnew"], gnew, floor, gnew_bound=bg)
                check_launch(tag + ("update",), cur, nxt, la, frozen=("var", "status", "gnew") + (() if small and live else ("grad",)))
            cur = nxt
            if special == "done" and it == 10:
                # the host rewrites EPS here (an ordinary state word) instead of starting with a large one, so that ten live steps
                # come first: EPS = twice the reference's max|gp| at this point, and the projection that follows must set DONE
                st = cur["st"].copy()
                st[R.EPS_W] = 2.0 * R.converged(st, cur["x"], cur["g"], 1.0, floor).state[R.GPSTATS + 1]
                rig.put(st=st)
                cur = rig.snap()
            if special == "done" or it % 5 == 4:
                rig.converged(1.0, floor)
                nxt = rig.snap()
                la = R.converged(cur["st"], cur["x"], cur["g"], 1.0, floor)
                if not R.idle(cur["st"]) and not la.extra["done_margin"] > 0:
                    la.state[R.DONE] = nxt["st"][R.DONE]             # max|gp| within its bound of EPS: either flag is right
                    la.written[R.DONE] = True
                check_launch(tag + ("converged",), cur, nxt, la, scratch=R.SCRATCH)
                cur = nxt
            if was_idle:
                saw_idle_launches = True                         # every launch of this iteration was checked to change nothing
    finally:
        rig.gate(False)
    st = cur["st"]
    if special == "fail":
        assert st[R.FAIL] == 1.0 and saw_idle_launches
    elif special == "done":
        assert st[R.DONE] == 1.0 and saw_idle_launches
    else:
        assert st[R.FAIL] == 0.0 and st[R.IT] >= 10
    assert undecidable <= UNDECIDABLE_CAP * max(decisions, 1), (name, undecidable, decisions)
    print("lockstep %s: it %d count %d decisions %d undecidable %d pending_seen %s" % (name, st[R.IT], st[R.COUNT], decisions, undecidable, saw_pending))
    if name == "small_o1":
        assert saw_pending and st[R.COUNT] > st[R.IT] + 1           # the run backtracks across a step boundary


@pytest.mark.gpu
@pytest.mark.parametrize("shape,n_out,slots", [("small", 3, 1), ("small", 3, 2), ("large", 1, 1), ("large", 8, 2)])
def test_window_equals_the_call_by_call_sequence(gpu, shape, n_out, slots):
    """bluest_spg_window(n_iterations = 20, check_last = 1) against the same launches issued one by one: every fold is in fixed
    order, so state and vectors agree bit for bit"""
    torch = gpu
    plan, scale, _ = _plan(shape, n_out)
    L, small, floor, N = plan.L, shape == "small", 1e-8, 20
    results = []
    for mode in ("calls", "window"):
        rig = Rig(torch, L, n_out, plan)
        rig.pws.zero_()                                          # both runs start from the same (cold) projection workspace
        _start(rig, plan, scale, n_out, 32.0, floor)
        rig.gate(True)
        try:
            if mode == "window":
                with torch.cuda.device(rig.dev):
                    rig.check(rig.lib.bluest_spg_window(plan._h, rig.p("x"), rig.p("g"), rig.p("d"), rig.p("xnew"), rig.p("m"), rig.p("scale"),
                                                        rig.p("st"), rig.p("var"), rig.p("status"), rig.p("grad"), rig.p("enable"),
                                                        rig.p("work"), rig.pws.data_ptr(), rig.v_ws, floor, slots, N, 1, rig.stream()))
            else:
                for it in range(N):
                    rig.direction(1.0, floor)
                    for t in range(slots):
                        if t > 0:
                            rig.trial()
                        rig.decide("eval_decide" if small else "eval_grad_decide", 1 if t == slots - 1 else 0)
                        torch.cuda.synchronize()
                    (rig.finish if small else rig.update_fused)(floor)
                rig.converged(1.0, floor)
            results.append(rig.snap())
        finally:
            rig.gate(False)
    a, b = results
    assert a["st"][R.IT] >= 5
    for k in ("st", "x", "g", "d", "xnew", "m", "var", "status", "grad", "enable"):
        assert np.array_equal(bits(a[k]), bits(b[k])), (shape, n_out, slots, k)

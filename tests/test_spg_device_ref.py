"""
CPU: anchors the restated device SPG machine (oracle/spg_device_ref.py).

1. Driven with the oracle's own V and grad V (floor 0, p = inf, one output, H = 10, the reference's lambda limits) it reproduces
   the recorded reference runs of tests/golden/spg_traj_*.npz -- with 1, 2 and 3 line-search slots per step, so the carry-over
   of a rejected last slot through PENDING does not change the algorithm.
2. Run in float64 (a model of the device arithmetic) on the shapes of the GPU lock-step test, at most 1 Armijo test in 20
   is closer to its threshold than the bounds of both sides: the cap the GPU test applies to the device.
"""
import numpy as np
import pytest

from bluest_amd import synth
from conftest import golden, rel_err
from oracle import spg_device_ref as ref

# the shapes of tests/test_gpu_spg_steps.py LOCKSTEP (name -> n, kmax, n_out, p, floor).  Its mapped plan (mapped_o3: the
# n = 20, k <= 5 groups with 30 % of them dropped per output) is the decision arithmetic of n20_k5_o8_p32 on fewer outputs
# (the oracle used here evaluates identity plans only), so it has no row of its own
LOCKSTEP_SHAPES = {
    "small_o1": (10, 3, 1, np.inf, 0.0),
    "small_o3_p32": (10, 3, 3, 32.0, 0.0),
    "small_o3_floor": (10, 3, 3, np.inf, 1e-8),
    "n20_k5_o1": (20, 5, 1, np.inf, 0.0),
    "n20_k5_o8_p32": (20, 5, 8, 32.0, 1e-8),
}
UNDECIDABLE_CAP = 1.0 / 20.0


def _evaluator(orc, n, kmax, n_out):
    prob = synth.problem(n, kmax, n_out)
    saps = [orc.OracleSAP(prob["C"][o], kmax, prob["groups"], prob["costs"]) for o in range(n_out)]
    scale = prob["budget"] / prob["costs"]

    def evaluate(m):
        var, status = np.zeros(n_out), np.zeros(n_out, dtype=np.int32)
        for o, sap in enumerate(saps):
            try:
                var[o] = sap.variance(m)
            except AssertionError:                     # the reference refuses the allocation: F = inf, a backtrack
                var[o], status[o] = np.inf, 1
        return var, status, (lambda: [sap.variance_GH(m, nohess=True)[1] for sap in saps])
    return evaluate, scale, saps[0].L


@pytest.mark.parametrize("slots", [1, 2, 3])
@pytest.mark.parametrize("fname", ["spg_traj_n6.npz", "spg_traj_n12_k4.npz"])
def test_machine_reproduces_the_recorded_reference_runs(oracle, fname, slots):
    G = golden(fname)
    n, kmax = int(G["n"]), int(G["kmax"])
    evaluate, scale, L = _evaluator(oracle, n, kmax, 1)
    fvals = []
    state, x, log = ref.run_machine(evaluate, np.ones(L) / L, scale, np.ones(1), p=np.inf, floor=0.0, H=10, lmin=1e-30, lmax=1e30,
                                    eps=float(G["eps"]), maxit=int(G["maxit"]), maxfev=10 ** 5, slots=slots, normalise=False,
                                    on_eval=lambda var: fvals.append(float(var[0])))
    assert int(state[ref.IT]) == int(G["it"]) and int(state[ref.COUNT]) == int(G["count"]), (state[ref.IT], state[ref.COUNT])
    assert len(fvals) == len(G["fvals"])
    fin = np.isfinite(G["fvals"])
    assert (np.isfinite(fvals) == fin).all()
    assert rel_err(np.array(fvals)[fin], G["fvals"][fin]) < 1e-9            # the bar of test_spg_trajectory
    assert rel_err(x, G["x"]) < 1e-6
    assert abs(state[ref.F] * state[ref.NORM] / float(G["f"]) - 1) < 1e-9
    if slots == 1 and int(G["count"]) > int(G["it"]) + 1:
        # every backtrack of a one-slot run crosses a step boundary: the PENDING branch of the direction was taken
        assert sum(1 for _, acc in log if not acc) == int(G["count"]) - 1 - int(G["it"])


@pytest.mark.parametrize("name", sorted(LOCKSTEP_SHAPES))
def test_undecidable_share_of_the_lockstep_shapes(oracle, name):
    """float64 against longdouble, 60 iterations, one slot: the steps whose Armijo margin (computed by the restatement in
    longdouble) is not positive are at most 1 in 20 in either run.  (The two runs are not compared step by step: they are free
    trajectories, whose rounding differences grow; that comparison is the GPU lock-step test's.)  Tried: synth.problem's default seed for every shape; no shape needed another one."""
    n, kmax, n_out, p, floor = LOCKSTEP_SHAPES[name]
    evaluate, scale, L = _evaluator(oracle, n, kmax, n_out)
    s_norm = np.ones(n_out)
    kw = dict(p=p, floor=floor, H=10, lmin=1e-30, lmax=1e3, eps=0.0, maxit=60, maxfev=10 ** 5, slots=1)
    _, _, log_ld = ref.run_machine(evaluate, np.ones(L) / L, scale, s_norm, wide=np.longdouble, **kw)
    _, _, log_64 = ref.run_machine(evaluate, np.ones(L) / L, scale, s_norm, wide=np.float64, **kw)
    for log in (log_ld, log_64):
        undecidable = sum(1 for margin, _ in log if not margin > 0)
        assert len(log) >= kw["maxit"] and undecidable <= UNDECIDABLE_CAP * len(log), (name, undecidable, len(log))

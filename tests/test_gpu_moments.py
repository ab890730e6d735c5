"""
GPU tests of bluest_amd.moments.MomentsMixin end to end: the tests/golden/estimator_case_*.npz fixtures replayed with MOSAP.solve set
to the recorded allocation, as tests/test_gpu_estimator.py replays them.  solve() keeps the bits of SamplingMixin.solve();
sample_moments is the covariance of the very samples that were drawn; with the model's blocks the new error bar is the one solve()
returns, and with the samples' it is the stated formula; values that stay on the device give the same bits.
"""
import numpy as np
import pytest

import gsums_ref
from gsums_ref import same_bits

pytestmark = pytest.mark.gpu

CASES = gsums_ref.case_names()
EPS = 2.0 ** -52


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    from bluest_amd.moments import MomentsMixin
    return MomentsMixin, SamplingMixin, BLUEProblem


def _solve_args(g):
    kw = dict(K=int(g["K"]), eps=float(g["eps"]))
    if "multi_groups" in g:
        kw["multi_groups"] = [[list(gr) for gr in mg] for mg in g["multi_groups"]]
    return kw


def cond_phi(g):
    """per output the condition number of Phi on its support, from numpy alone"""
    M, out = int(g["M"]), []
    for n in range(int(g["n_outputs"])):
        C = g["C"][n]
        mine = (lambda gr: True) if "multi_groups" not in g else (lambda gr, s={tuple(x) for x in g["multi_groups"][n]}: tuple(gr) in s)
        Phi = np.zeros((M, M))
        for gr, m in zip(g["groups"], g["samples"]):
            if m > 0 and mine(gr):
                Phi[np.ix_(gr, gr)] += m * np.linalg.inv(C[np.ix_(gr, gr)])
        idx = np.flatnonzero(np.diag(Phi) != 0)
        out.append(np.linalg.cond(Phi[np.ix_(idx, idx)]))
    return np.array(out)


@pytest.mark.parametrize("name", CASES)
def test_solve_keeps_its_bits_and_the_moments_are_those_of_the_draw(name, monkeypatch):
    from bluest_amd import mosap
    g = gsums_ref.case(name)
    monkeypatch.setattr(mosap.MOSAP, "solve", gsums_ref.fixed_allocation(g["samples"]))
    n_calls, n_out = int(g["solve_calls"]), int(g["n_outputs"])
    MomentsMixin, SamplingMixin, BLUEProblem = _classes()
    plain = gsums_ref.replay_class(g, SamplingMixin, BLUEProblem)()
    want = plain.solve(**_solve_args(g))
    p = gsums_ref.replay_class(g, MomentsMixin, SamplingMixin, BLUEProblem)()
    mus, errs, cost = p.solve(**_solve_args(g))
    assert p.calls == plain.calls == g["call_list"][:n_calls]
    assert same_bits(mus, want[0]) and same_bits(errs, want[1]) and cost == want[2]

    segs = gsums_ref.segments_of(g, 0, n_calls)
    chosen = np.flatnonzero(g["samples"] > 0).tolist()
    assert sorted(p.sample_moments) == chosen
    covs = {}
    for gi, (ls, v) in zip(chosen, segs):
        N, C = p.sample_moments[gi]
        assert N == v.shape[1] == int(g["samples"][gi]) and list(p.MOSAP_output["flattened_groups"][gi]) == ls
        if N >= 2:
            covs[gi] = np.array([np.cov(v[n].T).reshape(len(ls), len(ls)) for n in range(n_out)])
            assert np.allclose(C, covs[gi], rtol=1e-10, atol=0), (gi, ls)
        else:
            assert np.isnan(C).all()

    # the model's blocks give the promised error back
    allowed = np.maximum(1e-11, 50 * cond_phi(g) * EPS)
    model = p.sampled_errors(source="model")
    print(name, "sampled_errors(model) / errs - 1:", np.abs(model / errs - 1), "allowed", allowed)
    assert (np.abs(model / errs - 1) <= allowed).all()

    # the samples' covariances give the formula, evaluated by numpy on the same draws
    W = p._blue_weights()[0]
    var, c = np.zeros(n_out), 0
    for gi, (ls, v) in zip(chosen, segs):
        for n in range(n_out):
            w = W[n, c:c + len(ls)]
            C = covs[gi][n] if gi in covs else g["C"][n][np.ix_(ls, ls)]
            if w.any():
                var[n] += v.shape[1] * (w @ C @ w)
        c += len(ls)
    sampled = p.sampled_errors()
    print(name, "sampled_errors()", sampled, "promised", errs)
    assert np.allclose(sampled, np.sqrt(var), rtol=1e-10, atol=0)
    Cs, dofs = p.pooled_covariances()
    assert all(C.shape == (int(g["M"]),) * 2 and np.array_equal(C, C.T, equal_nan=True) for C in Cs) and all((d > 0).any() for d in dofs)

    # device-resident values: evaluate returns CUDA tensors, the same bits come out
    q = gsums_ref.replay_class(g, MomentsMixin, SamplingMixin, BLUEProblem)()
    q.on_device = True
    mus_dev, errs_dev, _ = q.solve(**_solve_args(g))
    assert q.calls == p.calls and same_bits(mus_dev, mus) and same_bits(errs_dev, errs)
    for gi in chosen:
        assert q.sample_moments[gi][0] == p.sample_moments[gi][0]
        assert np.array_equal(q.sample_moments[gi][1], p.sample_moments[gi][1], equal_nan=True)
    assert same_bits(q.sampled_errors(), sampled)

"""
GPU tests of the MLMC estimator (bluest_amd.mlmc.MLMCMixin: setup_mlmc / solve_mlmc / compute_mlmc_data; reference
bluest/blue_models.py:578-769) on top of the model-subset search kernel (csrc/mlmc.hip), against reference fixtures
(tools/gen_golden_mlmc.py).
"""
import glob
import os

import numpy as np
import pytest

from conftest import GOLDEN, golden

pytestmark = pytest.mark.gpu

CASES = sorted(os.path.basename(f)[5:-4] for f in glob.glob(os.path.join(GOLDEN, "mlmc_*.npz")) if "helpers" not in f)


def _rel(a, b):
    a, b = np.asarray(a, dtype=np.float64), np.asarray(b, dtype=np.float64)
    assert a.shape == b.shape
    return float(np.abs(a - b).max() / max(np.abs(b).max(), 1e-300)) if a.size else 0.0


def _class():
    from bluest_amd import BLUEProblem
    from bluest_amd.mlmc import MLMCMixin

    class P(MLMCMixin, BLUEProblem):
        pass
    return P


def _problem(C, w, dV=None, **kw):
    return _class()(len(w), C=list(C), costs=w, mlmc_variances=dV, n_outputs=len(C), verbose=False, **kw)


def _kwargs(g):
    kw = {"continuous_relaxation": bool(g["continuous_relaxation"])}
    if "budget" in g: kw["budget"] = float(g["budget"][0])
    else: kw["eps"] = [float(e) for e in g["eps"]] if len(g["eps"]) > 1 else float(g["eps"][0])
    return kw


def _same(d, g):
    assert [int(j) for j in d["models"]] == g["models"].tolist()
    s = np.asarray(d["samples"])
    assert s.dtype.kind == g["samples"].dtype.kind
    if s.dtype.kind == "i": assert np.array_equal(s, g["samples"])
    else: assert _rel(s, g["samples"]) < 1e-12
    assert _rel(d["errors"], g["errors"]) < 1e-12
    assert _rel(d["total_cost"], g["total_cost"]) < 1e-12


def test_fixture_list():
    assert len(CASES) == 20


@pytest.mark.parametrize("name", CASES)
def test_setup_mlmc_matches_reference(name):
    g = golden("mlmc_%s.npz" % name)
    P = _problem(g["C"], g["costs"], list(g["mlmc_variances"]) if "mlmc_variances" in g else None)
    d = P.setup_mlmc(**_kwargs(g))
    _same(d, g)
    cd = P.compute_mlmc_data(d["models"], d["samples"])
    assert _rel(cd["errors"], g["cd_errors"]) < 1e-12 and _rel(cd["total_cost"], g["cd_total_cost"]) < 1e-12


def test_eps_as_a_scalar_and_as_a_list():
    g = golden("mlmc_n8_eps.npz")
    P = _problem(g["C"], g["costs"])
    e = float(g["eps"][0])
    for eps in (e, [e], np.float64(e)):
        _same(P.setup_mlmc(eps=eps), g)
    _same(P.setup_mlmc(eps=e, budget=None), g)
    b = golden("mlmc_n8_budget.npz")
    _same(P.setup_mlmc(budget=float(b["budget"][0]), eps=123.0), b)           # the budget wins


class _Toy(object):
    """linear-Gaussian models on the telescoping covariance of a fixture: model j = mean_j + sum_{k >= j} sqrt(var_k) Z_k"""

    def __init__(self, g, seed):
        C = g["C"][0]
        tail = np.diag(C)
        self.sd = np.sqrt(np.concatenate([tail[:-1] - tail[1:], tail[-1:]]))
        self.mean = 1.0 + 0.1 * np.arange(len(tail))
        self.rng = np.random.RandomState(seed)
        self.calls = []


def _toy_problem(g, toy, **kw):
    from bluest_amd import BLUEProblem
    from bluest_amd.mlmc import MLMCMixin

    class P(MLMCMixin, BLUEProblem):
        def sampler(self, ls, N=1):
            Z = toy.rng.randn(len(toy.sd))
            return [Z for _ in ls]

        def evaluate(self, ls, samples, N=1):
            return [[toy.mean[l] + float(np.sum(toy.sd[l:] * samples[i][l:])) for i, l in enumerate(ls)]]

        def _group_sums(self, ls, N):
            toy.calls.append((list(ls), int(N)))
            return BLUEProblem._group_sums(self, ls, N)
    return P(len(g["costs"]), C=g["C"][0], costs=g["costs"], verbose=False, **kw)


def test_solve_mlmc_on_a_linear_gaussian_problem():
    g = golden("mlmc_n6_eps.npz")
    toy = _Toy(g, 11)
    P = _toy_problem(g, toy)
    eps = 20 * float(g["eps"][0])                                  # a few thousand model evaluations in all
    mu, errs, cost = P.solve_mlmc(eps=eps)
    d = P.setup_mlmc(eps=eps)
    gr, s = [int(j) for j in d["models"]], [int(x) for x in d["samples"]]
    assert len(gr) >= 2
    assert toy.calls == [([a, b], n) for a, b, n in zip(gr[:-1], gr[1:], s[:-1])] + [([gr[-1]], s[-1])]
    assert np.array_equal(errs, d["errors"]) and cost == d["total_cost"] and max(errs) <= eps * (1 + 1e-12)
    assert abs(mu[0] - toy.mean[0]) < 6 * errs[0]
    toy.calls.clear()
    mu2, errs2, cost2 = P.solve_mlmc(budget=123.0, mlmc_data=d)   # a given estimator is used as it is
    assert [c[1] for c in toy.calls] == s and abs(mu2[0] - toy.mean[0]) < 6 * errs[0] and cost2 == cost


def test_errors():
    from bluest_amd import BLUESTError
    g = golden("mlmc_n6_eps.npz")
    P = _problem(g["C"], g["costs"])
    with pytest.raises(BLUESTError, match="no group of models"):
        P.setup_mlmc(budget=0.9 * g["costs"][0])                   # NONE: not even one sample of model 0
    # 26 models coupled in a chain: the admissible groups are the prefixes, the largest has 26 levels
    n = 26
    var = 1.7 ** (-(n - 1.0 - np.arange(n)))
    tail = np.cumsum(var[::-1])[::-1]
    C = tail[np.maximum.outer(np.arange(n), np.arange(n))]
    far = np.abs(np.subtract.outer(np.arange(n), np.arange(n))) > 1
    C[far] = np.inf
    w = 1.5 ** (-np.arange(n, dtype=np.float64))
    P = _problem([C], w)
    with pytest.raises(ValueError, match="Too many dimensions"):
        P.setup_mlmc(eps=1e-3)
    d = P.setup_mlmc(eps=1e-3, continuous_relaxation=True)         # the same input answers without the rounding
    assert d["models"][0] == 0 and d["models"] == list(range(len(d["models"])))
    n = 32
    R = np.full((n, n), 0.5) + 0.5 * np.eye(n)
    with pytest.raises(BLUESTError, match="31 models below model 0"):
        _problem([R], np.linspace(1, 0.5, n)).setup_mlmc(eps=0.1)
    with pytest.raises(BLUESTError, match="not the first model in cost order"):
        _problem([R[:3, :3]], np.array([1.0, 1.0, 0.5])).setup_mlmc(eps=0.1)


def test_two_ranks_get_the_broadcast_result():
    """rank 0 searches and broadcasts; a rank that is not 0 never touches the GPU and returns what it was sent"""
    g = golden("mlmc_three_out_eps.npz")

    class Comm(object):
        def __init__(self, rank, box): self.rank, self.box = rank, box
        def Get_rank(self): return self.rank
        def Get_size(self): return 2

        def bcast(self, obj, root=0):
            if self.rank == root: self.box.append(obj)
            return obj if self.rank == root else self.box[-1]
        def allreduce(self, obj, op=None): return obj
        def barrier(self): return None
    box = []
    kw = _kwargs(g)
    d0 = _problem(g["C"], g["costs"], comm=Comm(0, box)).setup_mlmc(**kw)
    assert len(box) == 1 and box[0] is d0
    P1 = _problem(g["C"], g["costs"], comm=Comm(1, box))
    P1._mlmc_search = None                                         # calling it would raise: rank 1 must not search
    d1 = P1.setup_mlmc(**kw)
    assert d1 is d0
    _same(d1, g)

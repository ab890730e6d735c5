"""
Host tests of bluest_amd.estimator.SamplingMixin with group_sums replaced by its numpy restatement (tests/gsums_ref.py): the
sampler is called exactly as the reference called it in the tests/golden/estimator_case_*.npz fixtures (one-argument, batched and
batch-1 forms), non-finite batches are drawn again, the MPI split and gather, the host path of a class with its own inner
products, what BLUEProblem alone keeps refusing, and the rate of complexity_test.  The allocation and the weights are set by hand
here (the optimiser and the pseudo-inverse live on the GPU: tests/test_gpu_estimator.py).
"""
import numpy as np
import pytest

import gsums_ref

CASES = gsums_ref.case_names()


def _classes():
    from bluest_amd.blue_models import BLUEProblem
    from bluest_amd.estimator import SamplingMixin
    return SamplingMixin, BLUEProblem


@pytest.fixture
def stubbed(monkeypatch):
    """group_sums -> the restatement; every call's arguments are kept"""
    from bluest_amd import estimator
    seen = []

    def fake(values, weights=None, repeat_of=None, R=None, slab_bytes=None):
        seen.append((values, weights, repeat_of, R))
        return gsums_ref.group_sums(values, weights, repeat_of, R)
    monkeypatch.setattr(estimator, "group_sums", fake)
    return seen


def hand_set(p, g, seed=5):
    """put the fixture's allocation in place of setup_solver, and random weights in place of the GPU solve"""
    samples = np.asarray(g["samples"])
    chosen = np.flatnonzero(samples > 0)
    T = sum(len(g["groups"][i]) for i in chosen)
    W = np.random.RandomState(seed).randn(int(g["n_outputs"]), T)
    Vs = np.asarray(g["errs"]) ** 2
    out = {"budget": None, "eps": [float(g["eps"])] * int(g["n_outputs"]), "samples": samples, "flattened_groups": g["groups"],
           "variances": Vs, "cost": float(g["cost"])}
    p.MOSAP_output = out
    p.setup_solver = lambda **kw: out
    p._blue_weights = lambda: (W, Vs)
    return W


def test_fixtures_are_there():
    assert set(CASES) == {"one_arg", "batched", "ragged"}
    for name in CASES:
        g = gsums_ref.case(name)
        assert len(g["call_list"]) == (int(g["vt_N"]) + 1) * int(g["solve_calls"])
        ratio = g["vt_err"] / g["vt_err_ex"]
        assert ((ratio >= 0.6) & (ratio <= 1.5)).all()                  # the band holds for the reference itself
        assert (g["samples"] == 0).any() and 0 in {i for gr, m in zip(g["groups"], g["samples"]) if m > 0 for i in gr}
    b = gsums_ref.case("batched")
    counts, batch = set(b["samples"][b["samples"] > 0].tolist()), int(b["batch"])
    assert min(counts) < batch and batch in counts and max(counts) > batch


@pytest.mark.parametrize("name", CASES)
def test_group_sums_calls_the_sampler_as_the_reference_did(name, stubbed):
    g = gsums_ref.case(name)
    p = gsums_ref.replay_class(g, *_classes())()
    want = gsums_ref.segments_of(g, 0, int(g["solve_calls"]))
    for (ls, values), count in zip(want, g["samples"][g["samples"] > 0]):
        got = p._group_sums(ls, int(count))
        assert gsums_ref.same_bits(np.array(got), gsums_ref.segment_sums(values))
        assert np.allclose(np.array(got), values.sum(axis=1), rtol=1e-13)
    assert p.calls == g["call_list"][:int(g["solve_calls"])]
    assert len(stubbed) == len(want)                                    # one group_sums call per group
    assert p._group_sums([0, 1], 0) == [[0.0, 0.0]] * int(g["n_outputs"]) and len(p.calls) == int(g["solve_calls"])


@pytest.mark.parametrize("name", CASES)
def test_solve_and_variance_test_replay_the_whole_call_sequence(name, stubbed):
    g = gsums_ref.case(name)
    n_calls, N = int(g["solve_calls"]), int(g["vt_N"])
    p = gsums_ref.replay_class(g, *_classes())()
    W = hand_set(p, g)
    mus, errs, cost = p.solve(K=int(g["K"]), eps=float(g["eps"]))
    assert p.calls == g["call_list"][:n_calls] and len(stubbed) == 1   # ONE group_sums call for the whole estimator
    flat = np.concatenate([v.sum(axis=1) for _, v in gsums_ref.segments_of(g, 0, n_calls)], axis=1)
    assert np.allclose(mus, (W * flat).sum(axis=1), rtol=1e-12, atol=1e-12 * np.abs(W * flat).sum(axis=1).max())
    assert np.array_equal(errs, g["errs"]) and cost == float(g["cost"])
    err_ex, err = p.variance_test(eps=float(g["eps"]), K=int(g["K"]), N=N)
    assert p.calls == g["call_list"]                                    # the N repeats, in the reference's order
    assert len(stubbed) == 2 and stubbed[1][3] == N and list(stubbed[1][2]) == sorted(stubbed[1][2])
    per_repeat = []
    for r in range(N):
        flat = np.concatenate([v.sum(axis=1) for _, v in gsums_ref.segments_of(g, (r + 1) * n_calls, n_calls)], axis=1)
        per_repeat.append((W * flat).sum(axis=1))
    per_repeat = np.array(per_repeat)
    want = np.sqrt((per_repeat ** 2).sum(axis=0) / N - per_repeat.sum(axis=0) ** 2 / N**2)
    assert np.array_equal(err_ex, g["errs"]) and np.allclose(err, want, rtol=1e-9)


def test_a_flush_in_the_middle_of_a_repeat_changes_nothing(stubbed, monkeypatch):
    from bluest_amd import estimator
    g = gsums_ref.case("batched")
    P = gsums_ref.replay_class(g, *_classes())
    whole = P(start=int(g["solve_calls"]))
    hand_set(whole, g)
    one = whole._sample_estimators(3)
    n_whole = len(stubbed)
    monkeypatch.setattr(estimator, "SLAB_BYTES", 500)                   # a flush after every second or third group
    split = P(start=int(g["solve_calls"]))
    hand_set(split, g)
    several = split._sample_estimators(3)
    assert n_whole == 1 and len(stubbed) - n_whole > 3 and split.calls == whole.calls
    assert np.allclose(one, several, rtol=1e-13)                        # (the parts of a repeat's mu are added in order)
    assert any(c[3] == 2 for c in stubbed[n_whole:])                    # some flush begins in one repeat and ends in the next


def test_a_non_finite_batch_is_drawn_again(stubbed):
    SamplingMixin, BLUEProblem = _classes()

    class P(SamplingMixin, BLUEProblem):
        draws = 0

        def sampler(self, ls, N=1):
            self.draws += 1
            return [np.full(N, float(self.draws))] * len(ls)

        def evaluate(self, ls, samples, N=1):
            bad = self.draws in (2, 3)                                  # the second batch fails twice
            return [[np.where(bad & (np.arange(len(s)) == 1), np.nan if self.draws == 2 else np.inf, s + l) for s, l in zip(samples, ls)]]

    p = P(3, C=np.eye(3) + 0.5, costs=np.array([4.0, 2.0, 1.0]), verbose=False, sample_batch_size=4)
    got = p._group_sums([0, 2], 10)
    assert p.draws == 5                                                 # batches of 4, 4 (third try), 2
    assert got == [[4 * 1.0 + 4 * 4.0 + 2 * 5.0, 4 * 3.0 + 4 * 6.0 + 2 * 7.0]]


class FakeComm(object):
    """rank `rank` of `size`; gather and bcast talk through the board the ranks share (the root runs last)"""

    def __init__(self, rank, size, board):
        self.rank, self.size, self.board = rank, size, board

    def Get_rank(self): return self.rank
    def Get_size(self): return self.size
    def barrier(self): return None

    def gather(self, obj, root=0):
        self.board.setdefault("gather", {})[self.rank] = obj
        return [self.board["gather"][r] for r in range(self.size)] if self.rank == root else None

    def bcast(self, obj, root=0):
        if self.rank == root:
            self.board["bcast"] = obj
        return self.board.get("bcast")


def test_the_samples_are_split_over_the_ranks_and_gathered_on_rank_0(stubbed):
    SamplingMixin, BLUEProblem = _classes()

    class P(SamplingMixin, BLUEProblem):
        def sampler(self, ls, N=1):
            self.asked.append(N)
            return [100.0 * self.mpiRank + np.arange(N)] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[s + l for s, l in zip(samples, ls)], [2 * s for s in samples]]

    board, size, results = {}, 3, {}
    C = [np.eye(2) + 0.5] * 2
    for rank in (2, 1, 0):                                              # rank 0 last: it finds the others' shares gathered
        p = P(2, C=C, costs=np.array([2.0, 1.0]), n_outputs=2, verbose=False, sample_batch_size=3, comm=FakeComm(rank, size, board))
        p.asked = []
        results[rank] = (p._group_sums([0, 1], 11), p.asked)
    assert [results[r][1] for r in range(3)] == [[3, 1], [3, 1], [3]]  # 11 = 4 + 4 + 3, in batches of 3
    values = stubbed[0][0][0]
    assert values.shape == (2, 11, 2)
    assert values[0, :, 0].tolist() == [0, 1, 2, 0, 100, 101, 102, 100, 200, 201, 202]   # rank order, each rank in batches
    assert len(stubbed) == 1                                            # the kernel runs on rank 0 alone
    assert results[0][0] == [[float(values[0, :, 0].sum()), float(values[0, :, 1].sum())], [float(values[1, :, 0].sum())] * 2]


def test_a_class_with_its_own_inner_products_takes_the_host_path(stubbed):
    SamplingMixin, BLUEProblem = _classes()

    class P(SamplingMixin, BLUEProblem):
        k = 0

        def sampler(self, ls, N=1):
            self.k += 1
            return [self.k] * len(ls)

        def evaluate(self, ls, samples, N=1):
            return [[np.array([s + l, 2.0 * s]) for s, l in zip(samples, ls)]]

        def get_models_inner_products(self):
            return [lambda a, b: float(np.dot(a, b))]

    p = P(2, C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False, sample_batch_size=4)
    got = p._group_sums([0, 1], 3)
    assert not stubbed                                                  # vector outputs: added up on the host, one sample a call
    assert p.k == 3 and np.array_equal(got[0][0], [6.0, 12.0]) and np.array_equal(got[0][1], [9.0, 12.0])


def test_blueproblem_alone_still_refuses():
    from bluest_amd.sap import BLUESTError
    from bluest_amd.pilot import PilotMixin
    SamplingMixin, BLUEProblem = _classes()
    kw = dict(C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False)
    for cls in (BLUEProblem, type("P", (PilotMixin, BLUEProblem), {})):
        p = cls(2, **kw)
        with pytest.raises(BLUESTError):
            p.variance_test(eps=0.1)
        with pytest.raises(BLUESTError):
            p.complexity_test([0.1, 0.05])
    q = type("Q", (SamplingMixin, BLUEProblem), {})(2, **kw)
    with pytest.raises(BLUESTError):
        q.reorder_graph_nodes()
    with pytest.raises(ValueError):
        q.variance_test()                                               # neither a budget nor a tolerance


def test_complexity_test_fits_the_rate_of_the_costs():
    SamplingMixin, BLUEProblem = _classes()
    asked = []

    class P(SamplingMixin, BLUEProblem):
        def setup_solver(self, K=4, budget=None, eps=None, solver=None, **kw):
            asked.append((K, eps, solver))
            self.MOSAP_output = {"cost": 7.0 * eps ** -2}

    p = P(2, C=np.eye(2) + 0.5, costs=np.array([2.0, 1.0]), verbose=False)
    eps = [0.4, 0.2, 0.1, 0.05]
    tot_cost, rate = p.complexity_test(eps, K=2)
    assert asked == [(2, e, "spg") for e in eps]
    assert np.allclose(tot_cost, [7.0 * e ** -2 for e in eps]) and abs(rate - 2.0) < 1e-12


def test_group_sums_has_no_cpu_path():
    import torch
    if torch.cuda.is_available():
        pytest.skip("GPU present")
    from bluest_amd import _lib, estimator
    with pytest.raises(_lib.BluestHipError):
        estimator.group_sums([np.ones((1, 4, 2))])
    with pytest.raises(ValueError):
        estimator.group_sums([])
    with pytest.raises(ValueError):
        estimator.group_sums([np.ones((1, 4, 2)), np.ones((2, 4, 2))])

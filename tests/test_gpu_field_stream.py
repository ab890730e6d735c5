"""
GPU tests of StreamedFieldsMixin (bluest_amd.field_stream) on the real kernels: the problem of tests/test_field_stream_host.py with
CUDA batches against its unstreamed twin, bit for bit, in solve(), the sampled errors, field_sample_moments and variance_test;
solve_mc through _group_sums; and the one thing the mix-in is for -- a streamed solve() does not hold the group.
"""
import numpy as np
import pytest

from gsums_ref import same_bits
from test_field_stream_host import BATCH, SAMPLES, _bases, assert_twins, everything, hand_set, toy

pytestmark = pytest.mark.gpu


@pytest.mark.parametrize("cuda", [True, False])
def test_the_streamed_problem_is_its_unstreamed_twin_on_the_real_kernels(cuda, monkeypatch):
    from bluest_amd import field_stream, fields
    from bluest_amd.field_stream import StreamedFieldsMixin
    plain = toy(_bases(), cuda=cuda)
    hand_set(plain)
    want = everything(plain)
    made = []
    real = field_stream.FieldAccumulator
    monkeypatch.setattr(field_stream, "FieldAccumulator", lambda *a, **kw: made.append(real(*a, **kw)) or made[-1])
    for threshold in (0, 13440):                                        # every group streamed; the two large ones only
        del made[:]
        p = toy(_bases(StreamedFieldsMixin), cuda=cuda, field_stream_bytes=threshold)
        hand_set(p)
        assert_twins(everything(p), want)
        assert len(made) == (4 * 2 * 5 if threshold == 0 else 4 * 2 * 2)
    monkeypatch.setattr(fields, "SLAB_BYTES", 1)                        # a flush after every group: the twin flushes there too
    plain_flushed = toy(_bases(), cuda=cuda)                            # (a flush adds its part to mus, so where it falls shows in mus)
    hand_set(plain_flushed)
    want_flushed = everything(plain_flushed)
    for threshold in (0, 13440):
        q = toy(_bases(StreamedFieldsMixin), cuda=cuda, field_stream_bytes=threshold)
        hand_set(q)
        assert_twins(everything(q), want_flushed)
    assert len(plain.calls) == 4 * sum(-(-int(m) // BATCH) for m in SAMPLES) + 1


def test_solve_mc_through_group_sums():
    from bluest_amd.field_stream import StreamedFieldsMixin
    plain, p = toy(_bases(), cuda=True, poison=(2,)), toy(_bases(StreamedFieldsMixin), cuda=True, poison=(2,), field_stream_bytes=0)
    want, got = plain.solve_mc(budget=4.0 * 333), p.solve_mc(budget=4.0 * 333)
    assert p.calls == plain.calls == [([0], 50)] * 7 + [([0], 33)]
    assert isinstance(got[0][0], float) and same_bits(got[0][0], want[0][0]) and same_bits(got[0][1], want[0][1])
    assert same_bits(got[1], want[1]) and got[2] == want[2]
    assert abs(got[0][0] - 2.0) < 0.3


def test_a_streamed_solve_never_holds_the_group():
    """4000 samples of 3 models with 512 components in batches of 100: the segment is 49 MB.  The unstreamed twin holds at least all
    of it (and twice that while the batches are joined); the streamed solve() must stay below a quarter of it."""
    import torch
    from bluest_amd.field_stream import StreamedFieldsMixin
    N, L, d, batch = 4000, 3, 512, 100
    segment = N * L * d * 8

    def problem(*front, **kw):
        class P(*_bases(*front)):
            def output_weights(self): return [np.ones(d)]

            def sampler(self, ls, N=1):
                return [torch.randn(int(N), d, dtype=torch.float64, device="cuda", generator=self.gen)] * len(ls)

            def evaluate(self, ls, samples, N=1):
                return [[s * (1.0 + 0.1 * l) + l for l, s in zip(ls, samples)]]

        p = P(L, C=np.eye(L) + 0.5, costs=np.array([4.0, 2.0, 1.0]), verbose=False, sample_batch_size=batch, **kw)
        p.gen = torch.Generator(device="cuda")
        p.gen.manual_seed(7)
        W, Vs = np.array([[0.5, -0.25, 0.125]]) / N, np.array([0.01])
        out = {"budget": None, "eps": [0.1], "samples": np.array([N]), "flattened_groups": [[0, 1, 2]], "variances": Vs, "cost": 1.0}
        p.MOSAP_output, p.setup_solver, p._blue_weights = out, (lambda **kw: out), (lambda: (W, Vs))
        return p

    def peak_rise(p):
        torch.cuda.synchronize()
        torch.cuda.empty_cache()
        torch.cuda.reset_peak_memory_stats()
        before = torch.cuda.memory_allocated()
        result = p.solve(eps=[0.1])
        torch.cuda.synchronize()
        return torch.cuda.max_memory_allocated() - before, result

    held, want = peak_rise(problem())
    rise, got = peak_rise(problem(StreamedFieldsMixin, field_stream_bytes=0))
    print("segment", segment, "bytes; peak rise held", held, "streamed", rise)
    assert held >= segment
    assert rise < segment // 4
    assert same_bits(got[0][0], want[0][0]) and same_bits(got[1], want[1])
    p = problem(StreamedFieldsMixin, field_stream_bytes=0)
    p.solve(eps=[0.1])
    n_moments, var = p.field_sample_moments[0][0]
    assert n_moments == N and var.shape == (d,) and np.allclose(var, (0.5 - 0.25 * 1.1 + 0.125 * 1.2) ** 2 / N ** 2, rtol=0.2)

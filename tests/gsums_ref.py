"""numpy restatement of the summation order of bluest_group_sums (include/bluest_hip.h, Part 11): every addition in the order the
header states, so the result has the kernel's bits; the long-double sums and the rounding bound the results are held to; and the
reading of the tests/golden/estimator_*.npz fixtures (tools/gen_golden_estimator.py documents their layout)."""
import glob
import os

import numpy as np

from conftest import GOLDEN

CHUNK, CLASSES, LANES = 128, 8, 64
CLASS_ROWS = CHUNK // CLASSES
LD = np.longdouble
U = 2.0 ** -53


def chunk_sums(block):
    """[..., rows <= 128, L] -> [..., L]: eight classes of sixteen consecutive rows, each added in ascending order from +0.0,
    joined as ((q0 + q1) + (q2 + q3)) + ((q4 + q5) + (q6 + q7))"""
    rows = block.shape[-2]
    q = []
    for k in range(CLASSES):
        acc = np.zeros(block.shape[:-2] + block.shape[-1:])
        for r in range(k * CLASS_ROWS, min((k + 1) * CLASS_ROWS, rows)):
            acc = acc + block[..., r, :]
        q.append(acc)
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]))


def segment_sums(values):
    """[n_out, N, L] -> [n_out, L] with the kernel's bits: chunks of 128 samples, lane l adds the chunks l, l + 64, ... in
    ascending order from +0.0, then for off = 32 .. 1 lane l < off takes p[l] + p[l + off]; the result is lane 0's"""
    values = np.asarray(values, dtype=np.float64)
    n_out, N, L = values.shape
    p = [np.zeros((n_out, L)) for _ in range(LANES)]
    for c, start in enumerate(range(0, N, CHUNK)):
        p[c % LANES] = p[c % LANES] + chunk_sums(values[:, start:start + CHUNK, :])
    off = LANES // 2
    while off > 0:
        for l in range(off):
            p[l] = p[l] + p[l + off]
        off //= 2
    return p[0]


def fma(a, b, c):
    """round(a * b + c) with ONE rounding: the sum in exact rational arithmetic, then Python's correctly rounded conversion
    (ties to even) -- what the device's fma returns for finite operands"""
    from fractions import Fraction
    return float(Fraction(float(a)) * Fraction(float(b)) + Fraction(float(c)))


def group_sums(values, weights=None, repeat_of=None, R=None, slab_bytes=None):
    """stand-in for bluest_amd.estimator.group_sums with the same bits: sums per segment, and mu[r][n] = the fma chain over the
    columns of repeat r in ascending order from +0.0"""
    vals = [np.asarray(v.cpu().numpy() if hasattr(v, "data_ptr") else v, dtype=np.float64) for v in values]
    sums = [segment_sums(v) for v in vals]
    if weights is None:
        return sums
    n_out = vals[0].shape[0]
    flat = np.concatenate(sums, axis=1)
    weights = np.asarray(weights, dtype=np.float64)
    repeat_of = np.zeros(len(vals), dtype=np.int64) if repeat_of is None else np.asarray(repeat_of, dtype=np.int64)
    R = int(repeat_of[-1]) + 1 if R is None else int(R)
    mu = np.zeros((R, n_out))
    col = 0
    for s, v in enumerate(vals):
        for j in range(v.shape[2]):
            for n in range(n_out):
                mu[repeat_of[s], n] = fma(weights[n, col], flat[n, col], mu[repeat_of[s], n])
            col += 1
    return sums, mu


def sums_ld(values):
    """[n_out, L] in long double, and the sums of the absolute values the rounding bound is stated in"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    return Y.sum(axis=1), np.abs(Y).sum(axis=1)


def same_bits(a, b):
    a, b = np.ascontiguousarray(a, dtype=np.float64), np.ascontiguousarray(b, dtype=np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.int64), b.view(np.int64))


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def case_names():
    return sorted(os.path.basename(p)[len("estimator_case_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "estimator_case_*.npz")))


_cache = {}


def case(name):
    """the fixture with its calls split up: call_list [(ls, N2)], blocks[call] = what evaluate returned, [n_out, L] for scalar
    outputs (batch 1 or a one-argument sampler) else [n_out, L, N2]; solve_calls = how many of them belong to solve()"""
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, "estimator_case_%s.npz" % name)))
        n_out = int(g["n_outputs"])
        scalar = int(g["batch"]) == 1 or bool(g["one_arg"])
        calls, blocks, off = [], [], 0
        for row in g["calls"]:
            n2, L = int(row[0]), int(row[1])
            ls = [int(l) for l in row[2:2 + L]]
            shape = (n_out, L) if scalar else (n_out, L, max(n2, 1))
            size = int(np.prod(shape))
            blocks.append(g["values"][off:off + size].reshape(shape))
            off += size
            calls.append((ls, n2))
        assert off == g["values"].size
        g["call_list"], g["blocks"] = calls, blocks
        g["groups"] = [[int(i) for i in row if i >= 0] for row in g["flattened_groups"]]
        if "multi_groups_flat" in g:
            g["multi_groups"] = [[[int(i) for i in row[1:] if i >= 0] for row in g["multi_groups_flat"] if row[0] == n]
                                 for n in range(n_out)]
        _cache[name] = g
    return _cache[name]


def replay_class(g, *bases):
    """a problem class over `bases` whose sampler and evaluate replay the fixture from call `start` on: the sampler records its
    call and hands out the call's number, evaluate returns what the reference's evaluate returned for that call (as CUDA tensors
    when the instance has `on_device` set)"""
    scalar = int(g["batch"]) == 1 or bool(g["one_arg"])

    class Replay(*bases):
        on_device = False

        def __init__(self, start=0, **kw):
            self.calls, self.start = [], start
            args = dict(n_outputs=int(g["n_outputs"]), verbose=False, sample_batch_size=int(g["batch"]),
                        C=[c.copy() for c in g["C"]], costs=g["costs"].copy())
            args.update(kw)
            super().__init__(int(g["M"]), **args)

        def _next(self, ls, n2):
            self.calls.append(([int(l) for l in ls], n2))
            return [self.start + len(self.calls) - 1] * len(ls)

        def evaluate(self, ls, samples, N=1):
            block = g["blocks"][samples[0]]
            if self.on_device:
                import torch
                return [[torch.from_numpy(np.array(block[n, i])).cuda() for i in range(len(ls))] for n in range(block.shape[0])]
            if scalar:
                return [[float(block[n, i]) for i in range(len(ls))] for n in range(block.shape[0])]
            return [[block[n, i].copy() for i in range(len(ls))] for n in range(block.shape[0])]

    if bool(g["one_arg"]):
        Replay.sampler = lambda self, ls: self._next(ls, -1)
    else:
        Replay.sampler = lambda self, ls, N=1: self._next(ls, int(N))
    return Replay


def fixed_allocation(samples):
    """what the generator put in place of the reference's MOSAP.solve, for bluest_amd.mosap.MOSAP: the recorded allocation"""
    samples = np.asarray(samples, dtype=np.int64)

    def solve(self, budget=None, eps=None, **kw):
        self.samples = samples.copy()
        self.budget, self.eps = budget, eps
        self.tot_cost = self.samples @ self.costs
        for n in range(self.n_outputs):
            self.SAPS[n].samples = self.samples[self.mappings[n]]
        return self.samples
    return solve


def segments_of(g, first, count_calls):
    """the [n_out, N, L] arrays of the groups drawn by the calls first .. first + count_calls - 1, one per run of calls with
    the same models that adds up to the group's sample count"""
    out, k, end = [], first, first + count_calls
    samples = {tuple(gr): int(m) for gr, m in zip(g["groups"], g["samples"]) if m > 0}
    while k < end:
        ls = g["call_list"][k][0]
        need, parts = samples[tuple(ls)], []
        while need > 0:
            b = g["blocks"][k]
            b = b.reshape(b.shape[0], b.shape[1], -1)
            parts.append(b.transpose(0, 2, 1))
            need -= b.shape[2]
            k += 1
        assert need == 0
        out.append((ls, np.ascontiguousarray(np.concatenate(parts, axis=1))))
    return out

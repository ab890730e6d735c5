"""numpy restatement of the pilot statistics (sums in long double), of the estimates made of them and of the model-graph file
layout (bluest/blue_models.py:265-299, :326-346), and the replay of the tests/golden/pilot_case_*.npz fixtures
(tools/gen_golden_pilot.py documents their layout)."""
import glob
import os

import numpy as np

from conftest import GOLDEN

LD = np.longdouble


def sums_ld(values):
    """(sumse, sumsc, sumsd1, sumsd2) of values [n_out, N, L] in long double; the difference sums at i < j, 0 elsewhere"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    sumse = Y.sum(axis=1)
    sumsc = np.einsum("nsi,nsj->nij", Y, Y)
    D = Y[:, :, :, None] - Y[:, :, None, :]
    upper = np.triu(np.ones((Y.shape[2], Y.shape[2])), 1)
    return sumse, sumsc, D.sum(axis=1) * upper, (D * D).sum(axis=1) * upper


def abs_sums_ld(values):
    """the sums of the absolute values of the same terms: what the rounding bounds are stated in"""
    Y = np.asarray(values, dtype=np.float64).astype(LD)
    D = np.abs(Y[:, :, :, None] - Y[:, :, None, :])
    Y = np.abs(Y)
    return Y.sum(axis=1), np.einsum("nsi,nsj->nij", Y, Y), D.sum(axis=1), (D * D).sum(axis=1)


def pilot_statistics(values, differences=True, slab_bytes=None):
    """stand-in for bluest_amd.pilot.pilot_statistics: the long-double sums rounded to float64"""
    se, sc, d1, d2 = (np.asarray(a, dtype=np.float64) for a in sums_ld(values))
    return (se, sc, d1, d2) if differences else (se, sc, None, None)


def estimates(sumse, sumsc, sumsd1, sumsd2, N):
    """C_hat [n_out, L, L] and the difference variances (bluest/blue_models.py:333, :339)"""
    C_hat = sumsc / N - sumse[:, :, None] * sumse[:, None, :] / N**2
    return C_hat, sumsd2 / N - (sumsd1 / N) * (sumsd1 / N)


def fill(C_in, dV_in, ls, C_hat, dV_hat):
    """the estimate written where the reference writes it: unknown entries of coupled pairs (0 where |rho| < 1e-7), and the
    entries of dV that are not finite, i < j among the sampled models"""
    C, dV = np.array(C_in, dtype=np.float64), np.array(dV_in, dtype=np.float64)
    for n in range(C.shape[0]):
        for i, gi in enumerate(ls):
            for j, gj in enumerate(ls):
                if np.isnan(C_in[n][gi, gj]):
                    c = C_hat[n][i, j]
                    C[n, gi, gj] = 0.0 if abs(c / np.sqrt(C_hat[n][i, i] * C_hat[n][j, j])) < 1e-7 else c
                if i < j and not np.isfinite(dV_in[n][gi, gj]):
                    dV[n, gi, gj] = dV_hat[n][i, j]
    return C, dV


def as_get_covariance(C, remove_uncorrelated=True):
    """what get_covariance() shows of a complete covariance in the user's convention: NaN where not coupled"""
    out = np.array(C, dtype=np.float64)
    for n in range(out.shape[0]):
        never = np.isinf(out[n])
        if remove_uncorrelated:
            never |= (out[n] == 0.0)
        np.fill_diagonal(never, False)
        out[n][never] = np.nan
    return out


def adjacency(C, remove_uncorrelated=True):
    """the C<n> matrix of a model-graph file from a covariance in the user's convention"""
    C = np.array(C, dtype=np.float64)
    A = np.where(np.isinf(C), 0.0, np.where(C == 0.0, 0.0 if remove_uncorrelated else np.inf, C))
    return A


# ---- bounds -------------------------------------------------------------------------------------------------------------------
U = 2.0 ** -53


def cov_bound(values, N):
    """per entry: two summations of <= N terms each, in different orders -- 4 N u (sum|y_i y_j| / N + sum|y_i| sum|y_j| / N^2);
    the analogous bound for the difference variances"""
    ae, ac, ad1, ad2 = (np.asarray(a, dtype=np.float64) for a in abs_sums_ld(values))
    return (4 * N * U * (ac / N + ae[:, :, None] * ae[:, None, :] / N**2), 4 * N * U * (ad2 / N + ad1 * ad1 / N**2))


def scatter(g, bound):
    """a bound on the sampled models' pairs, placed at the models' numbers (0 elsewhere: given entries must match exactly)"""
    M, ls = int(g["M"]), g["ls"]
    out = np.zeros((bound.shape[0], M, M))
    out[np.ix_(range(bound.shape[0]), ls, ls)] = bound
    return out


def within(got, want, bound):
    got, want = np.asarray(got, dtype=np.float64), np.asarray(want, dtype=np.float64)
    assert np.array_equal(np.isnan(got), np.isnan(want))
    ok = np.isnan(want) | (np.abs(got - want) <= bound) | (got == want)
    assert ok.all(), (np.abs(got - want)[~ok], bound[~ok])


# ---- fixtures ------------------------------------------------------------------------------------------------------------------
def case_names():
    return sorted(os.path.basename(p)[len("pilot_case_"):-len(".npz")] for p in glob.glob(os.path.join(GOLDEN, "pilot_case_*.npz")))


_cache = {}


def case(name):
    if name not in _cache:
        g = dict(np.load(os.path.join(GOLDEN, "pilot_case_%s.npz" % name)))
        M, n_out = int(g["M"]), int(g["n_outputs"])
        vec = len(g["vec_weights"]) if "vec_weights" in g else 0
        scalar = int(g["batch"]) == 1 or bool(g["one_arg"])
        calls, blocks, off = [], [], 0
        for row in g["calls"]:
            n2, L = int(row[0]), int(row[1])
            ls = [int(l) for l in row[2:2 + L]]
            count = max(n2, 1)
            shape = (n_out, L, vec) if vec else ((n_out, L) if scalar else (n_out, L, count))
            size = int(np.prod(shape))
            blocks.append(g["values"][off:off + size].reshape(shape))
            off += size
            calls.append((ls, n2))
        assert off == g["values"].size
        g["call_list"], g["blocks"] = calls, blocks
        g["C_given"] = np.full((n_out, M, M), np.nan) if bool(g["C_none"]) else g["C_in"]
        g["dV_given"] = g["dV_in"] if "dV_in" in g else np.full((n_out, M, M), np.nan)
        g["n_cost_calls"] = 2 * M if bool(g["costs_none"]) else 0
        g["ls"] = [int(l) for l in np.flatnonzero(np.isnan(g["C_given"]).any(axis=(0, 2)))]
        _cache[name] = g
    return _cache[name]


def pilot_values(g):
    """the [n_out, N, L] array of the covariance-estimation samples of a scalar-output fixture, in the order they were drawn"""
    blocks = g["blocks"][g["n_cost_calls"]:]
    return np.concatenate([b.reshape(b.shape[0], b.shape[1], -1) for b in blocks], axis=2).transpose(0, 2, 1)


def replay_class(g, *bases):
    """a problem class over `bases` whose sampler and evaluate replay the fixture: the sampler records its call and hands out the
    call's number, evaluate returns what the reference's evaluate returned for that call"""
    scalar = int(g["batch"]) == 1 or bool(g["one_arg"])
    vec = "vec_weights" in g

    class Replay(*bases):
        def __init__(self, **kw):
            self.calls, self.last = [], 0
            args = dict(n_outputs=int(g["n_outputs"]), verbose=False, sample_batch_size=int(g["batch"]),
                        covariance_estimation_samples=int(g["N"]), skip_projection=bool(g["skip_projection"]))
            if not bool(g["C_none"]): args["C"] = [c.copy() for c in g["C_in"]]
            if not bool(g["costs_none"]): args["costs"] = g["costs_in"].copy()
            if "dV_in" in g: args["mlmc_variances"] = [d.copy() for d in g["dV_in"]]
            args.update(kw)
            super().__init__(int(g["M"]), **args)

        def _next(self, ls, n2):
            self.calls.append(([int(l) for l in ls], n2))
            return [len(self.calls) - 1] * len(ls)

        def evaluate(self, ls, samples, N=1):
            self.last = int(ls[0])
            block = g["blocks"][samples[0]]
            if vec or not scalar:
                return [[block[n, i].copy() for i in range(len(ls))] for n in range(block.shape[0])]
            return [[float(block[n, i]) for i in range(len(ls))] for n in range(block.shape[0])]

    if bool(g["one_arg"]):
        Replay.sampler = lambda self, ls: self._next(ls, -1)
    else:
        Replay.sampler = lambda self, ls, N=1: self._next(ls, int(N))
    if "cost_table" in g:
        Replay.cost = property(lambda self: float(g["cost_table"][self.last]))
    if vec:
        w = g["vec_weights"]
        Replay.get_models_inner_products = lambda self: [lambda a, b: float(np.dot(a * w, b)) for n in range(int(g["n_outputs"]))]
    return Replay


def unpadded(SG):
    return [[int(i) for i in row if i >= 0] for row in SG]

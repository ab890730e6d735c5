"""
Write tests/golden/estimator_case_*.npz: one solve() and one variance_test(N=50) of the REFERENCE (its package, imported through
oracle.gen_golden.import_reference()) on small problems with a seeded recording sampler.  Run where the reference tree exists:

    python tools/gen_golden_estimator.py

None of the reference's optimisation back-ends is installed, so MOSAP.solve is replaced IN THE REFERENCE PROCESS by a function
that sets a hand-picked integer allocation and its cost exactly as the real one does on return (bluest/mosap.py:317-322); the
reference's setup_solver, solve, compute_BLUE_estimators and variance_test then run natively.  C is the toy model's exact
covariance, so the allocation's promised error is the estimator's true one and the generator asserts that the variance test
of the reference itself lands in [0.6, 1.5] x err_ex.

Layout (tests/gsums_ref.py reads it back):
  M, n_outputs, K, batch, one_arg, eps, C [n_out, M, M], costs [M]
  multi_groups_flat   (ragged case only) rows [output, members padded with -1]
  flattened_groups    the reference's global group list, padded with -1; samples = the allocation over it
  calls   [n_calls, M + 2] int64: N2 (-1: the sampler takes no count), len(ls), ls padded with -1
  values  float64, the evaluate results flattened call by call, each as [output][model][sample]
  solve_calls         the first solve_calls calls belong to solve(), the rest to variance_test (N repeats of as many)
  mus, errs, cost     what solve() returned;  vt_N, vt_err_ex, vt_err: what variance_test returned
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")
VT_N = 50


def model(n, l, z, e):
    """output n of model l: mean 1.5, correlated through z, own noise e, a square so that the outputs differ in more than scale
    (the toy model of tools/gen_golden_pilot.py)"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def exact_covariance(M, n):
    """z, e_l independent standard normals: cov = a^2 b_l b_m + 2 d^2 + [l = m] a^2 c_l^2 (cov(z, z^2) = 0, var(z^2) = 2)"""
    a, d = 1 + 0.3 * n, 0.1 * n
    b, c = 0.9 ** np.arange(M), 0.1 * (np.arange(M) + 1)
    return a * a * np.outer(b, b) + 2 * d * d + np.diag(a * a * c * c)


def cases():
    return [dict(name="one_arg", M=4, n_outputs=1, K=3, batch=4, seed=31, one_arg=True, eps=0.2,
                 alloc={(0,): 2, (0, 1, 2): 3, (1, 3): 7, (3,): 12}),
            # counts below, at and above the batch size of 4; groups of every size with zero samples
            dict(name="batched", M=5, n_outputs=2, K=3, batch=4, seed=32, eps=0.2,
                 alloc={(0, 1, 2): 3, (0, 4): 4, (1, 2, 3): 6, (3, 4): 9, (4,): 13}),
            dict(name="ragged", M=5, n_outputs=2, K=3, batch=1, seed=33, eps=0.2,
                 multi_groups=[[[0], [0, 1], [1, 2, 3], [3, 4], [4]], [[0], [0, 2], [1, 2, 3], [2, 4], [4]]],
                 alloc={(0,): 2, (0, 1): 4, (0, 2): 3, (1, 2, 3): 5, (3, 4): 6, (4,): 8})]


def make_class(base, spec):
    M, n_out, batch = spec["M"], spec["n_outputs"], spec["batch"]

    class Ref(base):
        def __init__(self, **kw):
            self.rng = np.random.RandomState(spec["seed"])
            self.calls, self.vals = [], []
            super().__init__(M, n_outputs=n_out, verbose=False, sample_batch_size=batch, skip_projection=True, **kw)

        def _draw(self, ls, N):
            d = self.rng.randn(N, 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples):
            Ps = [[model(n, l, *samples[i]) for i, l in enumerate(ls)] for n in range(n_out)]
            if batch == 1 or spec.get("one_arg"):
                Ps = [[float(v[0]) for v in row] for row in Ps]
            self.vals.append(np.asarray(Ps, dtype=np.float64).ravel())
            return Ps

    if spec.get("one_arg"):
        def sampler(self, ls):
            self.calls.append(([int(l) for l in ls], -1))
            return self._draw(ls, 1)
    else:
        def sampler(self, ls, N=1):
            self.calls.append(([int(l) for l in ls], int(N)))
            return self._draw(ls, N)
    Ref.sampler = sampler
    return Ref


def padded(rows, width):
    return np.array([list(r) + [-1] * (width - len(r)) for r in rows], dtype=np.int64).reshape(len(rows), width)


def main():
    from oracle.gen_golden import import_reference
    _, bluest, _, _ = import_reference()
    from bluest import mosap as ref_mosap
    os.makedirs(OUT, exist_ok=True)
    for spec in cases():
        M, n_out = spec["M"], spec["n_outputs"]
        alloc = spec["alloc"]

        def fixed_solve(self, budget=None, eps=None, **kw):
            samples = np.array([alloc.get(tuple(int(i) for i in g), 0) for g in self.flattened_groups], dtype=np.int64)
            assert samples.sum() == sum(alloc.values()), "an allocated group is not in the group list"
            self.samples, self.budget, self.eps = samples, budget, eps
            self.tot_cost = samples @ self.costs
            for n in range(self.n_outputs):
                self.SAPS[n].samples = samples[self.mappings[n]]
            return samples

        ref_mosap.MOSAP.solve = fixed_solve
        C = [exact_covariance(M, n) for n in range(n_out)]
        costs = 2.0 ** -np.arange(M)
        P = make_class(bluest.BLUEProblem, spec)(C=[c.copy() for c in C], costs=costs.copy())
        kw = dict(K=spec["K"], eps=spec["eps"])
        if "multi_groups" in spec:
            kw["multi_groups"] = [[list(g) for g in mg] for mg in spec["multi_groups"]]
        mus, errs, cost = P.solve(**kw)
        solve_calls = len(P.calls)
        samples = np.array(P.MOSAP_output["samples"], dtype=np.int64)
        groups = [[int(i) for i in g] for g in P.MOSAP_output["flattened_groups"]]
        if "multi_groups" in spec:
            kw["multi_groups"] = [[list(g) for g in mg] for mg in spec["multi_groups"]]
        err_ex, err = P.variance_test(N=VT_N, **kw)
        assert len(P.calls) == (VT_N + 1) * solve_calls
        assert 0 in {i for g, m in zip(groups, samples) if m > 0 for i in g} and (samples == 0).any()
        ratio = np.asarray(err) / np.asarray(err_ex)
        assert ((ratio >= 0.6) & (ratio <= 1.5)).all(), ("the reference's own variance test leaves the band", ratio)
        rec = {"M": np.int64(M), "n_outputs": np.int64(n_out), "K": np.int64(spec["K"]), "batch": np.int64(spec["batch"]),
               "one_arg": np.bool_(spec.get("one_arg", False)), "eps": np.float64(spec["eps"]), "C": np.array(C), "costs": costs,
               "flattened_groups": padded(groups, M), "samples": samples,
               "calls": padded([[n2, len(ls)] + ls for ls, n2 in P.calls], M + 2), "values": np.concatenate(P.vals),
               "solve_calls": np.int64(solve_calls), "mus": np.array(mus, dtype=np.float64), "errs": np.array(errs, dtype=np.float64),
               "cost": np.float64(cost), "vt_N": np.int64(VT_N), "vt_err_ex": np.array(err_ex, dtype=np.float64),
               "vt_err": np.array(err, dtype=np.float64)}
        if "multi_groups" in spec:
            rec["multi_groups_flat"] = padded([[n] + list(g) for n, mg in enumerate(spec["multi_groups"]) for g in mg], M + 1)
        path = os.path.join(OUT, "estimator_case_%s.npz" % spec["name"])
        np.savez_compressed(path, **rec)
        print(spec["name"], len(P.calls), "calls,", rec["values"].size, "values,", os.path.getsize(path), "bytes, err / err_ex =", ratio)


if __name__ == "__main__":
    main()

"""
Write tests/golden/fields_estimator.npz: one solve() and one variance_test(N=20) of the REFERENCE (its package, imported through
oracle.gen_golden.import_reference()) on a problem whose second output is a vector of five components with the inner product
sum_c mass_c a_c b_c (get_models_inner_products written in Python, as in the reference's examples/multi_output_example.py).
Run where the reference tree exists:

    python tools/gen_golden_fields.py

As in tools/gen_golden_estimator.py, MOSAP.solve is replaced IN THE REFERENCE PROCESS by a function that sets a hand-picked
integer allocation; setup_solver, solve, compute_BLUE_estimators and variance_test of the reference then run natively, one
sample per sampler call.

Layout (tests/test_gpu_fields.py reads it back):
  M, n_outputs, K, eps [2], C [2, M, M], costs [M], mass [d], amp [d]
  flattened_groups    the reference's global group list, padded with -1; samples = the allocation over it
  calls   [n_calls, M + 2] int64: N2, len(ls), ls padded with -1
  values  float64, call by call: the number of every model, then the d components of every model
  solve_calls         the first solve_calls calls belong to solve(), the rest to variance_test (N repeats of as many)
  mu0, mu1 [d], errs, cost    what solve() returned;  vt_N, vt_err_ex, vt_err: what variance_test returned
"""
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden", "fields_estimator.npz")
M, K, VT_N, SEED = 4, 3, 20, 35
MASS = np.array([0.5, 1.0, 2.0, 1.0, 0.25])
AMP = np.array([1.0, -0.5, 2.0, 0.1, 3.0])
ALLOC = {(0,): 2, (0, 1, 2): 3, (1, 3): 7, (3,): 12}


def model(n, l, z, e):
    """the toy model of tools/gen_golden_estimator.py"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def exact_covariance(n):
    a, d = 1 + 0.3 * n, 0.1 * n
    b, c = 0.9 ** np.arange(M), 0.1 * (np.arange(M) + 1)
    return a * a * np.outer(b, b) + 2 * d * d + np.diag(a * a * c * c)


def main():
    from oracle.gen_golden import import_reference
    _, bluest, _, _ = import_reference()
    from bluest import mosap as ref_mosap

    def fixed_solve(self, budget=None, eps=None, **kw):
        samples = np.array([ALLOC.get(tuple(int(i) for i in g), 0) for g in self.flattened_groups], dtype=np.int64)
        assert samples.sum() == sum(ALLOC.values()), "an allocated group is not in the group list"
        self.samples, self.budget, self.eps = samples, budget, eps
        self.tot_cost = samples @ self.costs
        for n in range(self.n_outputs):
            self.SAPS[n].samples = samples[self.mappings[n]]
        return samples

    ref_mosap.MOSAP.solve = fixed_solve

    class Ref(bluest.BLUEProblem):
        def __init__(self, **kw):
            self.rng = np.random.RandomState(SEED)
            self.calls, self.vals = [], []
            super().__init__(M, n_outputs=2, verbose=False, sample_batch_size=1, skip_projection=True, **kw)

        def get_models_inner_products(self):
            return [lambda a, b: a * b, lambda a, b: float(np.dot(a * MASS, b))]

        def sampler(self, ls, N=1):
            self.calls.append(([int(l) for l in ls], int(N)))
            d = self.rng.randn(N, 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples):
            Ps = [[float(model(0, l, *samples[i])[0]) for i, l in enumerate(ls)],
                  [AMP * float(model(1, l, *samples[i])[0]) + np.arange(len(AMP)) for i, l in enumerate(ls)]]
            self.vals.append(np.concatenate([np.asarray(Ps[0]), np.asarray(Ps[1]).ravel()]))
            return Ps

    C = [exact_covariance(0), float(np.dot(AMP * MASS, AMP)) * exact_covariance(1)]
    eps = [0.25, 0.25 * float(np.sqrt(C[1][0, 0]))]
    costs = 2.0 ** -np.arange(M)
    P = Ref(C=[c.copy() for c in C], costs=costs.copy())
    mus, errs, cost = P.solve(K=K, eps=eps)
    solve_calls = len(P.calls)
    samples = np.array(P.MOSAP_output["samples"], dtype=np.int64)
    groups = [[int(i) for i in g] for g in P.MOSAP_output["flattened_groups"]]
    err_ex, err = P.variance_test(N=VT_N, K=K, eps=eps)
    assert len(P.calls) == (VT_N + 1) * solve_calls
    ratio = np.asarray(err) / np.asarray(err_ex)
    assert ((ratio >= 0.5) & (ratio <= 1.6)).all(), ("the reference's own variance test leaves the band", ratio)
    pad = lambda rows, width: np.array([list(r) + [-1] * (width - len(r)) for r in rows], dtype=np.int64).reshape(len(rows), width)
    rec = {"M": np.int64(M), "n_outputs": np.int64(2), "K": np.int64(K), "eps": np.array(eps), "C": np.array(C), "costs": costs,
           "mass": MASS, "amp": AMP, "flattened_groups": pad(groups, M), "samples": samples,
           "calls": pad([[n2, len(ls)] + ls for ls, n2 in P.calls], M + 2), "values": np.concatenate(P.vals),
           "solve_calls": np.int64(solve_calls), "mu0": np.float64(mus[0]), "mu1": np.array(mus[1], dtype=np.float64),
           "errs": np.array(errs, dtype=np.float64), "cost": np.float64(cost), "vt_N": np.int64(VT_N),
           "vt_err_ex": np.array(err_ex, dtype=np.float64), "vt_err": np.array(err, dtype=np.float64)}
    np.savez_compressed(OUT, **rec)
    print(len(P.calls), "calls,", rec["values"].size, "values,", os.path.getsize(OUT), "bytes, err / err_ex =", ratio, "mus", mus)


if __name__ == "__main__":
    main()

"""
Write tests/golden/covproj_*.npz: BLUEProblem.project_covariance(s) and the skip_projection=False constructor computed by the
REFERENCE (its package and native module, imported through oracle.gen_golden.import_reference()).  Run where the reference
tree exists:

    python tools/gen_golden_covproj.py

Each file holds one case:
  C (n_out x M x M)   the covariances given to the constructor (inf = never couple, 0 = uncorrelated)
  costs (M)           model costs
  verbose, remove_uncorrelated, skip_projection, bypass, maxit   constructor parameters / project_covariance argument
  call                0: project_covariance(n, bypass) for every output after construction; 1: nothing after construction
  raises              1 when the reference raised RuntimeError
  cov (n_out x M x M) get_covariances() afterwards (NaN = not coupled)
  err (n_out)         what project_covariance returned (NaN when not called)
  finite (n_out)      1 where every entry was known (the single clip), 0 where SPG ran
  it, count (n_out)   the SPG iteration / evaluation counts of the reference (-1 where SPG did not run), for information
"""
import contextlib
import io
import os
import sys

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")


def indefinite(M, seed, n_neg=2, neg=0.05, scale=1.0):
    """Q diag(l) Q^T with n_neg slightly negative eigenvalues, then scaled by random standard deviations"""
    rng = np.random.RandomState(seed)
    Q, _ = np.linalg.qr(rng.randn(M, M))
    l = rng.uniform(0.2, 2.0, M)
    l[:n_neg] = -neg * rng.uniform(0.5, 1.0, n_neg)
    C = Q @ np.diag(l) @ Q.T
    d = np.sqrt(np.abs(np.diag(C)))
    s = scale * rng.uniform(0.5, 2.0, M)
    C = C / np.outer(d, d) * np.outer(s, s)
    return (C + C.T) / 2


def uncouple(C, seed, frac=0.3):
    """set a random fraction of the pairs (i, j), 1 <= i < j, to inf (never coupled); model 0 stays coupled to every model"""
    rng = np.random.RandomState(seed + 1000)
    C = C.copy()
    M = C.shape[0]
    for i in range(1, M):
        for j in range(i + 1, M):
            if rng.rand() < frac:
                C[i, j] = C[j, i] = np.inf
    return C


def costs_of(M):
    return np.array([float(10 ** (3 - 3.0 * i / max(M - 1, 1))) for i in range(M)])


def run(bluest, Cs, costs, verbose=False, remove_uncorrelated=True, skip_projection=True, bypass=False, maxit=None, call=0):
    """build the reference problem, project, record; the reference's spg() is wrapped to record it / count"""
    import bluest.blue_models as bm
    records = []
    inner = bm.spg

    def spg_rec(*a, **k):
        res = inner(*a, **k)
        records.append((res["it"], res["count"]))
        return res
    bm.spg = spg_rec
    M, n_out = Cs[0].shape[0], len(Cs)
    params = {"verbose": verbose, "remove_uncorrelated": remove_uncorrelated, "skip_projection": skip_projection}
    if maxit is not None:
        params["spg_params"] = {"maxit": maxit}
    err = np.full(n_out, np.nan)
    it, count, finite = -np.ones(n_out, dtype=np.int64), -np.ones(n_out, dtype=np.int64), np.zeros(n_out, dtype=np.int64)
    raises = 0
    out = io.StringIO()
    prob = None
    try:
        with contextlib.redirect_stdout(out):
            try:
                prob = bluest.BLUEProblem(M, C=[c.copy() for c in Cs], costs=costs.copy(), n_outputs=n_out, **params)
                for n in range(n_out):
                    finite[n] = int(np.isfinite(prob.get_covariance(n)).all())
                if call == 0:
                    for n in range(n_out):
                        before = len(records)
                        err[n] = prob.project_covariance(n, bypass_error_check=bypass)
                        if len(records) > before:
                            it[n], count[n] = records[-1]
                else:
                    for n, r in enumerate(records):
                        it[n], count[n] = r
            except RuntimeError:
                raises = 1
    finally:
        bm.spg = inner
    cov = np.array(prob.get_covariances()) if prob is not None else np.full((n_out, M, M), np.nan)
    return dict(C=np.array(Cs), costs=costs, verbose=int(verbose), remove_uncorrelated=int(remove_uncorrelated),
                skip_projection=int(skip_projection), bypass=int(bypass), maxit=-1 if maxit is None else maxit, call=call,
                raises=raises, cov=cov, err=err, finite=finite, it=it, count=count, stdout=np.array(out.getvalue()))


def main():
    from oracle.gen_golden import import_reference
    _, bluest, _, _ = import_reference()
    cases = {}
    for M in (5, 12, 20):
        cases["finite_M%d" % M] = run(bluest, [indefinite(M, M)], costs_of(M))
    # a known zero kept coupled (remove_uncorrelated=False): the single clip replaces it too
    C = indefinite(6, 66)
    C[2, 4] = C[4, 2] = 0.0
    cases["finite_zero_M6"] = run(bluest, [C], costs_of(6), remove_uncorrelated=False)
    for M in (6, 12, 20):
        frac, neg = (0.3, 0.05) if M < 20 else (0.1, 0.2)
        cases["partial_M%d" % M] = run(bluest, [uncouple(indefinite(M, 100 + M, neg=neg), M, frac)], costs_of(M))
    cases["three_outputs_M8"] = run(bluest, [uncouple(indefinite(8, 201), 1, 0.2), indefinite(8, 202),
                                              uncouple(indefinite(8, 203, n_neg=1), 3, 0.5)], costs_of(8))
    # verbose: SPG ends above eps -> warning, covariance left as it was; bypass_error_check=True updates it
    P = uncouple(indefinite(7, 301, neg=0.2), 7)
    cases["early_return_M7"] = run(bluest, [P], costs_of(7), verbose=True)
    cases["bypass_M7"] = run(bluest, [P], costs_of(7), verbose=True, bypass=True)
    cases["maxit3_M6"] = run(bluest, [uncouple(indefinite(6, 106), 6)], costs_of(6), maxit=3)
    # the constructor path: inf = never coupled, 0 = a known zero, projected BEFORE the uncorrelated pairs are dropped
    C = uncouple(indefinite(9, 401), 9, 0.25)
    C[1, 5] = C[5, 1] = 0.0
    C[3, 7] = C[7, 3] = 0.0
    cases["constructor_M9"] = run(bluest, [C], costs_of(9), skip_projection=False, call=1)
    for name, d in cases.items():
        np.savez(os.path.join(OUT, "covproj_%s.npz" % name), **d)
        print("%-22s raises=%d err=%s it=%s count=%s" % (name, d["raises"], d["err"], d["it"], d["count"]))


if __name__ == "__main__":
    main()

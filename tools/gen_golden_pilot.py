"""
Write tests/golden/pilot_*.npz: the covariance / MLMC-variance / cost estimation and the model-graph files of the REFERENCE
(its package, imported through oracle.gen_golden.import_reference()).  Run where the reference tree exists:

    python tools/gen_golden_pilot.py

pilot_case_<name>.npz   a reference BLUEProblem subclass with a seeded sampler: its constructor arguments, every (ls, N) sampler
                        call, every value evaluate returned, and the resulting get_covariances(), get_mlmc_variances(),
                        get_costs() and SG.  Layout (tests/pilot_ref.py reads it back):
                          calls   [n_calls, M + 2] int64: N2 (-1: the sampler takes no count), len(ls), ls padded with -1
                          values  float64, the evaluate results flattened call by call, each as [output][model][sample or component]
                          C_in / C_none, costs_in / costs_none, dV_in (optional), cost_table (optional: problem.cost of the model
                          evaluated last), batch, N, skip_projection, vec_weights (optional: the weighted dot of vector outputs)
                          fn_sumse, fn_sumsc, fn_sumsd1, fn_sumsd2: what blue_fn(compute_mlmc_differences=True) returned
                          cov, dV, costs, SG (padded with -1); cov_skip = cov of the same run with skip_projection=True
pilot_graph_<paper>.npz three model-graph files the reference's paper drivers wrote, copied byte for byte
pilot_loaded.npz        what the reference's loader returns for each of them: plain, with `costs=` overridden, with fewer outputs
pilot_save.npz          the arrays of the file the reference's save_graph_data writes for one complete-C problem, key by key
"""
import os
import shutil
import sys
import tempfile

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
OUT = os.path.join(ROOT, "tests", "golden")

PAPER = {"hh": "hodgkin-huxley/model_graph_data.npz", "ns": "navier_stokes/NS_model_data_full.npz",
         "matern": "restrictions_matern/restrictions_matern_model_data.npz"}
VEC_WEIGHTS = np.array([1.0, 0.5, 2.0])


def model(n, l, z, e):
    """output n of model l: mean 1.5, correlated through z, own noise e, a square so that the outputs differ in more than scale"""
    return 1.5 + (1 + 0.3 * n) * (0.9 ** l * z + 0.1 * (l + 1) * e) + 0.1 * n * z ** 2


def make_class(base, spec):
    M, n_out, batch = spec["M"], spec["n_outputs"], spec["batch"]

    class Ref(base):
        def __init__(self, **kw):
            self.rng = np.random.RandomState(spec["seed"])
            self.calls, self.vals, self.last = [], [], 0
            super().__init__(M, n_outputs=n_out, verbose=False, sample_batch_size=batch,
                             covariance_estimation_samples=spec["N"], **kw)

        def blue_fn(self, ls, N, verbose=True, compute_mlmc_differences=False):
            out = super().blue_fn(ls, N, verbose=verbose, compute_mlmc_differences=compute_mlmc_differences)
            if compute_mlmc_differences: self.sums = out
            return out

        def _draw(self, ls, N):
            d = self.rng.randn(N, 1 + len(ls))
            return [(d[:, 0], d[:, 1 + i]) for i in range(len(ls))]

        def evaluate(self, ls, samples):
            self.last = int(ls[0])
            Ps = [[model(n, l, *samples[i]) for i, l in enumerate(ls)] for n in range(n_out)]
            if batch == 1 or spec.get("one_arg"):
                Ps = [[float(v[0]) for v in row] for row in Ps]
            if spec.get("vector"):
                Ps = [[np.array([v, 0.5 * v * v, np.sin(v)]) for v in row] for row in Ps]
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
    if "cost_table" in spec:
        Ref.cost = property(lambda self: spec["cost_table"][self.last])
    if spec.get("vector"):
        Ref.get_models_inner_products = lambda self: [lambda a, b: float(np.dot(a * VEC_WEIGHTS, b)) for n in range(n_out)]
    return Ref


def pattern(M, n_out, seed):
    """covariances with unknown (NaN) entries in every row, some pairs never coupled (inf), one uncorrelated (0), the rest given"""
    rng = np.random.RandomState(seed)
    Cs = []
    for n in range(n_out):
        A = rng.randn(M, M)
        C = A @ A.T / M + np.eye(M)
        K = np.full((M, M), np.nan)
        for i in range(M):
            K[i, i] = C[i, i] if (i + n) % 2 else np.nan
            j = (i + 2) % M
            K[i, j] = K[j, i] = C[i, j]
        K[0, M - 1] = K[M - 1, 0] = np.inf
        K[1, M - 2] = K[M - 2, 1] = np.inf if n == 0 else np.nan
        K[0, 3] = K[3, 0] = 0.0
        Cs.append(K)
    return Cs


def cases():
    w6 = 2.0 ** -np.arange(6)
    out = [dict(name="none_2out", M=6, n_outputs=2, N=50, batch=7, seed=11, costs=w6, skip_projection=True),
           dict(name="partial", M=6, n_outputs=2, N=40, batch=4, seed=12, costs=w6, skip_projection=True, C=pattern(6, 2, 3)),
           dict(name="costs_none", M=5, n_outputs=2, N=24, batch=5, seed=13, skip_projection=True,
                cost_table=np.array([7.0, 3.5, 2.0, 0.5, 0.25])),
           dict(name="batch1", M=4, n_outputs=2, N=16, batch=1, seed=14, costs=w6[:4], skip_projection=True),
           dict(name="one_arg", M=4, n_outputs=1, N=12, batch=6, seed=15, costs=w6[:4], skip_projection=True, one_arg=True),
           dict(name="projected", M=5, n_outputs=2, N=30, batch=8, seed=16, costs=w6[:5], skip_projection=False,
                C=pattern(5, 2, 4)),
           dict(name="dV_given", M=5, n_outputs=2, N=20, batch=6, seed=17, costs=w6[:5], skip_projection=True),
           dict(name="inner", M=4, n_outputs=2, N=14, batch=1, seed=18, costs=w6[:4], skip_projection=True, vector=True)]
    dV = [np.full((5, 5), np.nan) for _ in range(2)]
    dV[0][0, 1], dV[0][2, 4], dV[1][1, 3], dV[1][0, 4] = 0.125, 3.0, 0.75, np.inf
    out[6]["dV"] = dV
    return out


def padded(rows, width):
    return np.array([list(r) + [-1] * (width - len(r)) for r in rows], dtype=np.int64).reshape(len(rows), width)


def run_case(bluest, spec, skip_projection):
    kw = dict(skip_projection=skip_projection)
    if "C" in spec: kw["C"] = [c.copy() for c in spec["C"]]
    if "costs" in spec: kw["costs"] = np.array(spec["costs"])
    if "dV" in spec: kw["mlmc_variances"] = [d.copy() for d in spec["dV"]]
    return make_class(bluest.BLUEProblem, spec)(**kw)


def main():
    from oracle.gen_golden import import_reference, REF
    _, bluest, _, _ = import_reference()
    os.makedirs(OUT, exist_ok=True)
    for spec in cases():
        P = run_case(bluest, spec, spec["skip_projection"])
        M = spec["M"]
        rec = {"M": np.int64(M), "n_outputs": np.int64(spec["n_outputs"]), "N": np.int64(spec["N"]), "batch": np.int64(spec["batch"]),
               "skip_projection": np.bool_(spec["skip_projection"]), "one_arg": np.bool_(spec.get("one_arg", False)),
               "calls": padded([[n2, len(ls)] + ls for ls, n2 in P.calls], M + 2), "values": np.concatenate(P.vals),
               "cov": np.array(P.get_covariances()), "dV": np.array(P.get_mlmc_variances()), "costs": P.get_costs(),
               "SG": padded([sorted(int(i) for i in sg) for sg in P.SG], M)}
        se, sc, _, d1, d2 = P.sums            # what the reference's blue_fn(compute_mlmc_differences=True) returned
        zero = np.zeros_like(np.asarray(se[0][0], dtype=np.float64))
        rec["fn_sumse"], rec["fn_sumsc"] = np.array(se, dtype=np.float64), np.array(sc, dtype=np.float64)
        rec["fn_sumsd1"] = np.array([[[zero + v for v in row] for row in out] for out in d1], dtype=np.float64)
        rec["fn_sumsd2"] = np.array(d2, dtype=np.float64)
        rec["C_none"] = np.bool_("C" not in spec)
        if "C" in spec: rec["C_in"] = np.array(spec["C"])
        rec["costs_none"] = np.bool_("costs" not in spec)
        if "costs" in spec: rec["costs_in"] = np.array(spec["costs"])
        if "dV" in spec: rec["dV_in"] = np.array(spec["dV"])
        if "cost_table" in spec: rec["cost_table"] = spec["cost_table"]
        if spec.get("vector"): rec["vec_weights"] = VEC_WEIGHTS
        if not spec["skip_projection"]:
            Q = run_case(bluest, spec, True)
            assert [c for c in Q.calls] == [c for c in P.calls]
            rec["cov_skip"] = np.array(Q.get_covariances())
        np.savez(os.path.join(OUT, "pilot_case_%s.npz" % spec["name"]), **rec)
        print(spec["name"], len(P.calls), "calls,", rec["values"].size, "values")

    # the paper drivers' model-graph files, and what the reference's loader makes of them
    loaded = {}
    for tag, rel in PAPER.items():
        dst = os.path.join(OUT, "pilot_graph_%s.npz" % tag)
        shutil.copyfile(os.path.join(REF, "examples", "paper_examples", rel), dst)
        os.chmod(dst, 0o644)
        M, n_file = int(np.load(dst)["M"]), int(np.load(dst)["n_outputs"])
        variants = {"plain": dict(n_outputs=n_file), "costs": dict(n_outputs=n_file, costs=np.arange(M, 0, -1.0) ** 2),
                    "fewer": dict(n_outputs=max(n_file - 2, 1))}
        if n_file == 1: del variants["fewer"]
        for v, kw in variants.items():
            P = bluest.BLUEProblem(M, datafile=dst, verbose=False, **kw)
            pre = "%s_%s_" % (tag, v)
            loaded[pre + "n_outputs"] = np.int64(kw["n_outputs"])
            if "costs" in kw: loaded[pre + "costs_in"] = kw["costs"]
            loaded[pre + "cov"], loaded[pre + "dV"] = np.array(P.get_covariances()), np.array(P.get_mlmc_variances())
            loaded[pre + "costs"], loaded[pre + "SG"] = P.get_costs(), np.array(P.SG, dtype=np.int64)
    np.savez_compressed(os.path.join(OUT, "pilot_loaded.npz"), **loaded)

    # the file the reference writes for one complete-C problem (an inf, a zero and a finite mlmc_variances entry in it)
    rng = np.random.RandomState(21)
    Cs = []
    for n in range(2):
        A = rng.randn(5, 5)
        C = A @ A.T / 5 + np.eye(5)
        C[0, 4] = C[4, 0] = np.inf
        C[1, 3] = C[3, 1] = 0.0
        Cs.append(C)
    dV = [np.full((5, 5), np.nan) for _ in range(2)]
    dV[0][0, 1], dV[1][2, 3] = 0.5, 0.25
    costs = 2.0 ** -np.arange(5)
    P = bluest.BLUEProblem(5, C=[c.copy() for c in Cs], costs=costs, mlmc_variances=[d.copy() for d in dV], n_outputs=2,
                           verbose=False, skip_projection=True)
    with tempfile.TemporaryDirectory() as tmp:
        P.save_graph_data(os.path.join(tmp, "graph.npz"))
        data = dict(np.load(os.path.join(tmp, "graph.npz")))
    rec = {"in_C": np.array(Cs), "in_costs": costs, "in_dV": np.array(dV)}
    rec.update({"file_" + k: v for k, v in data.items()})
    np.savez(os.path.join(OUT, "pilot_save.npz"), **rec)
    print("save keys:", sorted(data))


if __name__ == "__main__":
    main()

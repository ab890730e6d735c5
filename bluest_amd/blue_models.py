"""
BLUEProblem -- the user-facing entry of the sample-allocation path: the signatures and return values
of `setup_solver()` / `solve()` of bluest/blue_models.py:448-576, on top of bluest_amd.mosap.MOSAP.

In scope here: given covariances and model costs -> model groups (cliques of the coupling graph up to size K, or the user's
groups), their union over the outputs, group costs, one MOSAP on the GPU, `solver="spg"`, the reference's return dictionaries;
`solve()` then samples the selected groups through the user's `sampler` / `evaluate` and forms the BLUE estimators.
The projection of the covariances onto the SPD matrices (`project_covariance(s)`, bluest/blue_models.py:348-433) is in scope:
the eigendecompositions and the whole SPG solve run on the GPU (bluest_cov_project, one workgroup per output).  The
constructor runs it only when asked (`skip_projection=False`; the default here is True, the reference's is False).
Refused by this class alone, with BLUESTError, and provided by opt-in mix-ins: estimating covariances, MLMC variances or costs by
sampling (C=None, NaN entries, costs=None) and saving / loading model graphs (bluest_amd.pilot.PilotMixin, through the hooks
_init_from_datafile / _init_inputs / _complete_inputs below), the MLMC driver (bluest_amd.mlmc.MLMCMixin), and batched sampling
with complexity_test / variance_test (bluest_amd.estimator.SamplingMixin, which replaces _group_sums and solve).  Out of scope for
all of them: sample files, reorder_graph_nodes.  MFMC (setup_mfmc / solve_mfmc / compute_mfmc_data, the subset search on the
GPU) and plain Monte Carlo (solve_mc) are in scope.  An MPI communicator passed
as `comm` is honoured the way the reference uses it (optimiser, estimators and projection on rank 0 + bcast, samples split
over the ranks).

Conventions kept from the reference (bluest/blue_models.py:43-56, :166-179): in a user covariance an infinite entry means "never
couple these two models", a zero entry means "uncorrelated" (such pairs are not coupled either when `remove_uncorrelated`, the
default); `get_covariance()` returns NaN where two models are not coupled.  Models that cannot be reached from model 0 through
couplings are left out of every group (:312-322).

A quirk of the reference kept on purpose (:403-409): when the SPG projection ends with an objective above spg_params["eps"]
and the problem is verbose, project_covariance() prints a warning and returns the error WITHOUT updating the covariance,
unless bypass_error_check=True; a problem that is not verbose is always updated.
"""
import ctypes

import numpy as np

from . import _lib, misc
from .mosap import MOSAP
from .host import in_host_section
from .sap import BLUESTError

BLUEST_MFMC_MAX_NEIGHBOURS = 30      # include/bluest_hip.h, Part 7
BLUEST_MFMC_TOO_BIG = 2

BLUEST_COVPROJ_MAXIT, BLUEST_COVPROJ_MAXFEV, BLUEST_COVPROJ_NONFINITE = 1, 2, 3     # include/bluest_hip.h, Part 8
BLUEST_MAX_MODELS = 64

spg_default_params = {"maxit": 10000,                    # bluest/blue_models.py:10-17
                      "max_fevals": 10000**2,
                      "verbose": False,
                      "spd_threshold": 5.0e-14,
                      "eps": 1.0e-10,
                      "lmbda_min": 10.**-30,
                      "lmbda_max": 10.**30,
                      "linesearch_history_length": 10,
                      }

default_params = {"verbose": True, "comm": None, "remove_uncorrelated": True, "optimization_solver": "spg", "sample_batch_size": 1,
                  "skip_projection": True, "spg_params": spg_default_params}


def cov_project(Cs, masks, spg_params):
    """bluest_cov_project on a list of M x M covariances and 0/1 masks (1 = known entry): per output (X, f, gpmax, it, count,
    info), the reference's spg() result fields, or the single clip (f = Frobenius error) where the mask is all ones"""
    Cs = np.ascontiguousarray(np.array(Cs, dtype=np.float64))
    masks = np.ascontiguousarray(np.array(masks, dtype=np.float64))
    n_out, M = Cs.shape[0], Cs.shape[1]
    X = np.empty_like(Cs)
    f, gpmax = np.zeros(n_out), np.zeros(n_out)
    it, count = np.zeros(n_out, dtype=np.int64), np.zeros(n_out, dtype=np.int64)
    info = np.zeros(n_out, dtype=np.int32)
    p = spg_params
    _lib.check(_lib.lib().bluest_cov_project(M, n_out, _lib.ptr(Cs), _lib.ptr(masks), float(p["spd_threshold"]), float(p["eps"]),
                                             float(p["lmbda_min"]), float(p["lmbda_max"]), int(p["maxit"]), int(p["max_fevals"]),
                                             int(p["linesearch_history_length"]), _lib.ptr(X), _lib.ptr(f), _lib.ptr(gpmax),
                                             _lib.ptr(it), _lib.ptr(count), _lib.ptr(info), None))
    return [(X[n], float(f[n]), float(gpmax[n]), int(it[n]), int(count[n]), int(info[n])) for n in range(n_out)]


class _SerialComm(object):
    """what `get_comm()` returns when no MPI communicator was passed (the reference defaults to mpi4py's COMM_WORLD,
    bluest/blue_models.py:22; mpi4py is not a dependency of this build): one rank, collectives are identities"""

    def Get_rank(self): return 0
    def Get_size(self): return 1
    def bcast(self, obj, root=0): return obj
    def allreduce(self, obj, op=None): return obj
    def barrier(self): return None
    def gather(self, obj, root=0): return [obj]


class _Coupling(object):
    """coupling structure of ONE output: the covariance and which pairs of models may share a group"""

    def __init__(self, C, remove_uncorrelated, unknown_ok=False):
        """unknown_ok (bluest_amd.pilot.PilotMixin): a NaN entry is a coupled pair whose covariance is still to be estimated"""
        C = np.array(C, dtype=np.float64)
        M = C.shape[0]
        if C.shape != (M, M):
            raise ValueError("covariance must be square")
        if np.isnan(C).any() and not unknown_ok:
            raise BLUESTError("unknown (NaN) covariance entries would have to be estimated by sampling and projected to SPD "
                              "(bluest/blue_models.py:326-433): outside this GPU build -- pass complete covariances")
        never = np.isinf(C)
        self.cov = np.where(never, 0.0, C)
        self.linked = ~never
        np.fill_diagonal(self.linked, True)
        self.linked &= self.linked.T
        self.check(remove_uncorrelated)

    def check(self, remove_uncorrelated):
        """drop the uncorrelated (zero) pairs when asked and find model 0's component (bluest/blue_models.py:305-322)"""
        if remove_uncorrelated:
            self.linked &= (self.cov != 0.0)
            np.fill_diagonal(self.linked, True)
        # models reachable from model 0
        seen, frontier = {0}, [0]
        while frontier:
            nxt = []
            for i in frontier:
                for j in np.flatnonzero(self.linked[i]).tolist():
                    if j not in seen:
                        seen.add(j)
                        nxt.append(j)
            frontier = nxt
        self.component = sorted(seen)

    @classmethod
    def from_adjacency(cls, A, component):
        """from a matrix of a model-graph file (bluest/blue_models.py:265-299): 0 = not coupled, inf = coupled and uncorrelated,
        anything else the covariance of a coupled pair; the component of model 0 is the file's"""
        self = cls.__new__(cls)
        A = np.array(A, dtype=np.float64)
        self.linked = A != 0.0
        self.cov = np.where(np.isinf(A) | ~self.linked, 0.0, A)
        self.component = [int(i) for i in component]
        return self

    def adjacency(self):
        """the matrix a model-graph file holds for this output"""
        return np.where(self.linked, np.where(self.cov == 0.0, np.inf, self.cov), 0.0)

    def update(self, C_new):
        """the projected covariance on the coupled pairs (bluest/blue_models.py:423-431); which pairs are coupled is unchanged"""
        self.cov = np.where(self.linked, C_new, self.cov)

    def covariance(self):
        out = self.cov.copy()
        out[~self.linked] = np.nan
        return out

    def is_clique(self, group):
        g = np.asarray(group, dtype=np.int64)
        return bool(self.linked[np.ix_(g, g)].all()) and all(int(i) in set(self.component) for i in g)

    def cliques(self, K):
        """all cliques of up to K models inside model 0's component, per size, each sorted, lexicographic order.  One size at a
        time over all its cliques: a (k-1)-clique c extends by every model j > c[-1] linked to all of c; the candidates are a
        64-bit mask per clique (the AND of the members' masks of linked larger models), and numpy.nonzero over the
        (clique, j) bit matrix lists the extensions row-major -- parent first, j ascending -- which keeps the order lexicographic"""
        nodes = np.asarray(self.component, dtype=np.int64)
        n = len(nodes)
        sub = self.linked[np.ix_(nodes, nodes)]
        bit = np.left_shift(np.uint64(1), np.arange(n, dtype=np.uint64))
        higher = np.array([np.bitwise_or.reduce(bit[(np.arange(n) > i) & sub[i]], initial=np.uint64(0)) for i in range(n)],
                          dtype=np.uint64)
        rows = np.arange(n, dtype=np.int64).reshape(-1, 1)         # local indices (nodes is ascending: same order as the models)
        cand = higher.copy()
        out = [rows]
        for k in range(2, K + 1):
            ext = ((cand[:, None] & bit[None, :]) != 0)
            parent, j = np.nonzero(ext)
            rows = np.concatenate([rows[parent], j[:, None].astype(np.int64)], axis=1)
            cand = cand[parent] & higher[j]
            out.append(rows)
        return [nodes[r].reshape(-1, k + 1) for k, r in enumerate(out)]


class BLUEProblem(object):
    def __init__(self, M, C=None, costs=None, mlmc_variances=None, datafile=None, n_outputs=1, **params):
        self.M, self.n_outputs = int(M), int(n_outputs)
        spg_params = dict(spg_default_params)                  # merged as bluest/blue_models.py:64-67
        spg_params.update(params.get("spg_params", {}))
        params["spg_params"] = spg_params
        self.params = dict(default_params, **params)
        self.default_params = default_params
        comm = self.params["comm"]
        if comm is None:
            comm = _SerialComm()
        self.mpiRank = comm.Get_rank()
        self.mpiSize = comm.Get_size()
        self.comm = comm
        self.warning = self.mpiRank == 0
        self.verbose = bool(self.params["verbose"]) and self.warning
        self.MOSAP = None
        self.MOSAP_output = None
        if datafile is not None:
            self._init_from_datafile(datafile, costs)
            return
        C, costs = self._init_inputs(C, costs)
        Cs = list(C) if isinstance(C, (list, tuple)) else [C]
        if len(Cs) != self.n_outputs or any(np.shape(c) != (self.M, self.M) for c in Cs):
            raise ValueError("need one %d x %d covariance per output" % (self.M, self.M))
        if mlmc_variances is None:                             # bluest/blue_models.py:77-92
            dV = [np.nan * np.ones((self.M, self.M)) for n in range(self.n_outputs)]
        else:
            dV = mlmc_variances
        self.dV = dV if isinstance(dV, (list, tuple)) else [dV]
        self._costs = np.array(costs, dtype=np.float64)
        if self._costs.shape != (self.M,):
            raise ValueError("costs must have one entry per model")
        project = not self.params["skip_projection"]
        self._coupling = [_Coupling(c, self.params["remove_uncorrelated"] and not project, self._unknown_ok) for c in Cs]
        self._complete_inputs()
        if project:                    # the reference's order (:94-101): project on the user's pattern, then drop uncorrelated pairs
            self.project_covariances()
            for cp in self._coupling:
                cp.check(self.params["remove_uncorrelated"])
        self.SG = [cp.component for cp in self._coupling]
        for n, cp in enumerate(self._coupling):
            if len(cp.component) < self.M and self.warning:
                print("WARNING! Model graph %d is not connected. Connected graph size: %d" % (n, len(cp.component)))
        self.check_costs(warning=True)
        if self.verbose: print("\nBLUE estimator ready.\n")

    # ---- the three places where this class refuses what bluest_amd.pilot.PilotMixin provides ----------------------------------
    _unknown_ok = False                                        # NaN covariance entries: _Coupling refuses them

    def _init_from_datafile(self, datafile, costs):
        raise BLUESTError("model-graph files (bluest/blue_models.py:265-299) are outside this GPU build: pass C and costs")

    def _init_inputs(self, C, costs):
        if C is None or costs is None:
            raise BLUESTError("covariances and costs must be given: estimating them by sampling (bluest/blue_models.py:326-346, "
                              ":435-441) is outside this GPU build")
        return C, costs

    def _complete_inputs(self):
        """between the coupling graphs and the projection: nothing to do when everything was given"""

    # ---- supplied by the user (bluest/blue_models.py:105-119) -----------------------------------------------------------------
    def evaluate(self, ls, samples, N=1):
        raise NotImplementedError("subclass BLUEProblem and implement evaluate(ls, samples)")

    def sampler(self, ls, N=1):
        raise NotImplementedError("subclass BLUEProblem and implement sampler(ls)")

    def get_models_inner_products(self):
        return [lambda a, b: a * b for n in range(self.n_outputs)]

    def get_comm(self):
        return self.comm

    # ---- data access ----------------------------------------------------------------------------------------------------------
    def get_costs(self):
        return self._costs.copy()

    def get_group_costs(self, groups):
        """cost of a group = sum of the costs of its models (bluest/blue_models.py:137-140); one entry per group, size-major"""
        parts = [self._costs[np.asarray(gk, dtype=np.int64).reshape(len(gk), -1)].sum(axis=1) for gk in groups if len(gk)]
        return np.concatenate(parts) if parts else np.zeros(0)

    def check_costs(self, warning=True):
        dearer = np.flatnonzero(self._costs > self._costs[0]).tolist()
        if dearer:
            if not warning:
                raise ValueError("Model zero is not the most expensive model. Consider removing the more expensive models %s" % dearer)
            if self.warning:
                print("WARNING! Model zero is not the most expensive model. The more expensive models are: %s" % dearer)
        return dearer

    def get_covariance(self, n=0):
        return self._coupling[n].covariance()

    def get_covariances(self):
        return [cp.covariance() for cp in self._coupling]

    def get_mlmc_variances(self):
        return self.dV

    def get_mlmc_variance(self, n=0):
        return self.dV[n]

    def get_correlation(self, n=0):
        C = self.get_covariance(n)
        sd = np.sqrt(np.diag(C))
        return C / np.outer(sd, sd)

    def get_correlations(self):
        return [self.get_correlation(n) for n in range(self.n_outputs)]

    # ---- groups ---------------------------------------------------------------------------------------------------------------
    def _groups_per_output(self, K, multi_groups):
        """per output: list over sizes of (L_k, k) int arrays, empty trailing sizes dropped; and the largest size per output"""
        per_output = []
        for n, cp in enumerate(self._coupling):
            if multi_groups is None:
                levels = cp.cliques(min(int(K), self.M))
            else:
                kept = sorted({tuple(sorted(int(i) for i in g)) for g in multi_groups[n] if len(g)})
                kept = [g for g in kept if cp.is_clique(g)]
                if not kept:
                    raise ValueError("no admissible model group for output %d" % n)
                kmax = max(len(g) for g in kept)
                levels = [np.array([g for g in kept if len(g) == k], dtype=np.int64).reshape(-1, k) for k in range(1, kmax + 1)]
            while levels and len(levels[-1]) == 0:
                levels.pop()
            per_output.append(levels)
        return per_output, [len(levels) for levels in per_output]

    @staticmethod
    def _union(per_output, K):
        """the global group list: union over the outputs per size, sorted (bluest/blue_models.py:491-501, hashed)"""
        first = per_output[0]
        if all(len(lv) == len(first) and all(np.array_equal(a, b) for a, b in zip(lv, first)) for lv in per_output[1:]):
            return [lv.copy() for lv in first] + [np.zeros((0, k), dtype=np.int64) for k in range(len(first) + 1, K + 1)]
        out = []
        for k in range(1, K + 1):
            rows = {tuple(r) for lv in per_output if len(lv) >= k for r in lv[k - 1].tolist()}
            out.append(np.array(sorted(rows), dtype=np.int64).reshape(-1, k))
        return out

    # ---- the path -------------------------------------------------------------------------------------------------------------
    @in_host_section
    def setup_solver(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, continuous_relaxation=False,
                     max_model_samples=None, optimization_solver_params=None):
        """bluest/blue_models.py:448-538: returns {"models", "samples", "errors", "total_cost"}"""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        if budget is not None:
            eps = None                                                  # the budget wins (bluest/blue_models.py:450)
        elif np.isscalar(eps):
            eps = [eps] * self.n_outputs
        solver = self.params["optimization_solver"] if solver is None else solver
        if multi_groups is not None and len(multi_groups) != self.n_outputs:
            raise ValueError("multi_groups must be a list of groupings of the same length as the number of outputs.")
        if multi_groups is None and groups is not None:
            multi_groups = [groups] * self.n_outputs
        per_output, Ks = self._groups_per_output(K, multi_groups)
        K = max(Ks)
        union = self._union(per_output, K)
        costs = self.get_group_costs(union)
        multi_costs = [self.get_group_costs(levels) for levels in per_output]
        C = self.get_covariances()

        if self.verbose: print("Computing optimal sample allocation...")
        result = None
        if self.mpiRank == 0:                                           # the optimiser runs on one rank (:508)
            self.MOSAP = MOSAP(C, K, Ks, union, per_output, costs, multi_costs, verbose=self.verbose)
            self.MOSAP.solve(eps=eps, budget=budget, solver=solver, continuous_relaxation=continuous_relaxation,
                             max_model_samples=max_model_samples, solver_params=optimization_solver_params)
            if self.MOSAP.samples is not None:
                Vs = self.MOSAP.variances(self.MOSAP.samples)
                result = {"budget": budget, "eps": eps, "samples": self.MOSAP.samples, "flattened_groups": self.MOSAP.flattened_groups,
                          "variances": Vs, "cost": self.MOSAP.tot_cost}
                if self.verbose:
                    cost_MC = max(C[n][0, 0] / Vs[n] for n in range(self.n_outputs)) * costs[0]
                    print("\nBLUE cost: ", result["cost"], "MC cost: ", cost_MC, "Savings: ", cost_MC / result["cost"])
        result = self.comm.bcast(result, root=0)                        # :526
        self.MOSAP_output = result
        if result is None:
            raise BLUESTError("MOSAP solution failed!")

        chosen = np.flatnonzero(result["samples"] > 0)
        data = {"models": [result["flattened_groups"][i] for i in chosen], "samples": result["samples"][chosen].copy(),
                "errors": np.sqrt(result["variances"]), "total_cost": result["cost"]}
        if self.verbose:
            print("\nModel groups selected: %s\n" % data["models"])
            print("BLUE estimator setup. Max error: ", np.sqrt(max(result["variances"])), " Cost: ", result["cost"], "\n")
        return data

    def _group_sums(self, ls, N):
        """sum over N joint samples of the models `ls`, per output: [n_outputs][len(ls)] (what bluest/blue_fn.py returns first).
        Host Python around the user's model -- sampling is not part of the accelerated path.  With an MPI communicator of
        several ranks the N samples are split as the reference splits them (blue_fn.py:107-111: N // size each, the first
        N % size ranks one more) and the sums are all-reduced (:178-182), so every rank returns the sums of all N."""
        comm = self.get_comm()
        size, rank = comm.Get_size(), comm.Get_rank()
        mine = int(N) // size + (1 if rank < int(N) % size else 0)
        sums = [[0 for _ in ls] for _ in range(self.n_outputs)]
        for _ in range(mine):
            while True:
                values = self.evaluate(ls, self.sampler(ls))
                if all(np.all(np.isfinite(v)) for out in values for v in out):
                    break                                               # non-finite model output: draw again (blue_fn.py:118-129)
            for n in range(self.n_outputs):
                for i in range(len(ls)):
                    sums[n][i] = sums[n][i] + values[n][i]
        if size > 1:
            for n in range(self.n_outputs):
                for i in range(len(ls)):
                    sums[n][i] = comm.allreduce(sums[n][i])            # default op of mpi4py's allreduce is SUM
        return sums

    def solve(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, verbose=True, continuous_relaxation=False,
              max_model_samples=None, optimization_solver_params=None):
        """bluest/blue_models.py:540-576: returns (estimates, their standard errors, total cost)"""
        have = self.MOSAP_output
        changed = have is not None and ((budget is not None and budget != have["budget"]) or
                                        (eps is not None and np.any(np.asarray(eps) != np.asarray(have["eps"]))))
        if have is None or changed:
            self.setup_solver(K=K, budget=budget, eps=eps, groups=groups, multi_groups=multi_groups, solver=solver,
                              continuous_relaxation=continuous_relaxation, max_model_samples=max_model_samples,
                              optimization_solver_params=optimization_solver_params)
        if self.verbose and verbose: print("\nSampling BLUE...\n")
        out = self.MOSAP_output
        sums = [[] for _ in range(self.n_outputs)]
        for ls, count in zip(out["flattened_groups"], out["samples"]):
            got = self._group_sums(ls, count) if count > 0 else [[0] * len(ls)] * self.n_outputs
            for n in range(self.n_outputs):
                sums[n].append(got[n])
        if self.mpiRank == 0:                                           # only rank 0 owns a MOSAP (:565-571)
            mus, Vs = self.MOSAP.compute_BLUE_estimators(sums, out["samples"])
        else:
            mus, Vs = None, None
        mus = self.comm.bcast(mus, root=0)
        Vs = self.comm.bcast(Vs, root=0)
        return mus, np.sqrt(Vs), out["cost"]

    # ---- MFMC and plain Monte Carlo (bluest/blue_models.py:773-930) ------------------------------------------------------------
    def _mfmc_inputs(self):
        sigmas = [np.sqrt(np.diag(self.get_covariance(n))) for n in range(self.n_outputs)]
        rhos = [self.get_correlation(n)[0, :] for n in range(self.n_outputs)]
        return sigmas, rhos, self.get_costs()

    def compute_mfmc_data(self, clique, samples):
        """bluest/blue_models.py:773-795: the MFMC estimator of the group `clique` (model 0 first) with the given samples"""
        sigmas, rhos, w = self._mfmc_inputs()
        clique = list(clique)
        if not all(cp.is_clique(clique) for cp in self._coupling):
            raise ValueError("Group given is not a clique of the model graph!")
        if clique[0] != 0:
            raise ValueError("The high-fidelity model, model 0, should be the first in the given group!")
        data = []
        for n in range(self.n_outputs):
            feasible, d = misc.compute_mfmc_data(sigmas[n][clique], rhos[n][clique], w[clique], samples)
            if not feasible:
                raise ValueError("Prescribed samples are not feasible for MFMC")
            data.append(d)
        return {"models": clique, "samples": samples, "errors": [d["error"] for d in data],
                "total_cost": max(d["total_cost"] for d in data), "alphas": [d["alphas"] for d in data]}

    @in_host_section
    def setup_mfmc(self, budget=None, eps=None, continuous_relaxation=False, small_budget=False):
        """bluest/blue_models.py:797-865: the best MFMC estimator over every clique through model 0 of the intersection of the
        coupling graphs, searched on the GPU (bluest_mfmc_search).  Returns {"models", "samples", "errors", "total_cost",
        "alphas"}; `models` is listed in the order the estimator uses (decreasing |rho|), and so are `samples` and `alphas`.
        BLUESTError when the outputs order the selected models differently."""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if eps is not None and np.isscalar(eps): eps = [eps for n in range(self.n_outputs)]
        if eps is None: eps = [None for n in range(self.n_outputs)]
        sigmas, rhos, w = self._mfmc_inputs()
        if self.verbose: print("Setting up optimal MFMC estimator...\n")
        data = None
        if self.mpiRank == 0:
            data = self._mfmc_search(sigmas, rhos, w, budget, eps, continuous_relaxation, small_budget)
            if self.verbose: print("Best MFMC estimator found. Coupled models:", data["models"], " Max error: ", max(data["errors"]),
                                   " Cost: ", data["total_cost"], "\n")
        return self.comm.bcast(data, root=0)

    def _mfmc_search(self, sigmas, rhos, w, budget, eps, continuous_relaxation, small_budget):
        linked = np.logical_and.reduce([cp.linked for cp in self._coupling])     # nx.intersection_all(self.G)
        nbrs = [j for j in np.flatnonzero(linked[0]).tolist() if j != 0]
        if len(nbrs) > BLUEST_MFMC_MAX_NEIGHBOURS:
            raise BLUESTError("model 0 has %d neighbours: the MFMC search covers at most %d (2^%d subsets)"
                              % (len(nbrs), BLUEST_MFMC_MAX_NEIGHBOURS, BLUEST_MFMC_MAX_NEIGHBOURS))
        local = np.array([0] + nbrs, dtype=np.int64)
        nb, n_out = len(nbrs), self.n_outputs
        s = np.ascontiguousarray([sg[local] for sg in sigmas], dtype=np.float64)
        rho = np.ascontiguousarray([r[local] for r in rhos], dtype=np.float64)
        perm = np.ascontiguousarray([misc.mfmc_order(r) for r in rho], dtype=np.int32)
        adj = np.array([sum(1 << (q - 1) for q in range(1, nb + 1) if q != p and linked[local[p], local[q]])
                        for p in range(1, nb + 1)], dtype=np.uint32)
        flags = (1 if budget is not None else 0) | (2 if continuous_relaxation else 0) | (4 if small_budget else 0)
        eps2 = None if budget is not None else np.array([e**2 for e in eps], dtype=np.float64)
        epsm2 = None if budget is not None else np.array([e**-2 for e in eps], dtype=np.float64)
        wl = np.ascontiguousarray(w[local], dtype=np.float64)
        mask, obj, status = ctypes.c_uint32(0), ctypes.c_double(0.0), ctypes.c_int32(0)
        combo = np.zeros(n_out, dtype=np.uint32)
        _lib.check(_lib.lib().bluest_mfmc_search(nb, n_out, flags, float(budget or 0.0), _lib.ptr(eps2), _lib.ptr(epsm2),
                                                 _lib.ptr(wl), _lib.ptr(s), _lib.ptr(rho), _lib.ptr(perm), _lib.ptr(adj),
                                                 ctypes.byref(mask), _lib.ptr(combo), ctypes.byref(obj), ctypes.byref(status),
                                                 None))
        if status.value == BLUEST_MFMC_TOO_BIG:
            raise ValueError('Too many dimensions to brute-force it')
        if status.value != 0:
            raise BLUESTError("no group of models admits an MFMC estimator")
        clique = [int(local[p]) for p in range(nb + 1) if p == 0 or (mask.value >> (p - 1)) & 1]
        # every output's samples in its own |rho| order, then the element-wise maximum per model (blue_models.py:859)
        per_output = []
        for n in range(n_out):
            cl = np.array(clique)
            feasible, idx, m, variance, alphas = misc.mfmc_allocation(sigmas[n][cl], rhos[n][cl], w[cl], budget=budget, eps=eps[n])
            assert feasible
            if not continuous_relaxation:
                if small_budget and budget is not None:
                    m = misc.mfmc_low_budget_integer_solution(rhos[n][cl][idx], w[cl][idx], budget)
                else:
                    m = misc.mfmc_round_from_combo(m, combo[n])
            per_output.append((cl[idx], m, variance, alphas))
        models = [int(j) for j in per_output[0][0]]
        if any(list(order) != models for order, _, _, _ in per_output[1:]):
            # one MFMC estimator nests the samples of every output in ONE order; the reference would pair each output's samples
            # and alphas with another output's order here, and report errors that do not describe what solve_mfmc computes
            raise BLUESTError("the outputs order the selected models %s differently by |rho| (%s): MFMC needs one nesting order "
                              "for all outputs" % (models, [[int(j) for j in order] for order, _, _, _ in per_output]))
        samples = np.max(np.vstack([m for _, m, _, _ in per_output]), axis=0)
        wm = w[models]
        cost = samples @ wm
        if budget is not None:          # adjust if budget bound (blue_models.py:850-854); the max takes care of the variance bound
            samples = np.floor(samples - (max(cost - budget, 0) / (wm @ wm)) * wm).astype(np.int64)
            samples[0] = max(samples[0], 1)
            cost = samples @ wm
        errs = [np.sqrt(variance(samples)) for _, _, variance, _ in per_output]
        alphas = [al for _, _, _, al in per_output]
        return {"models": models, "samples": samples, "errors": errs, "total_cost": cost, "alphas": alphas}

    def solve_mfmc(self, budget=None, eps=None, mfmc_data=None, continuous_relaxation=False):
        """bluest/blue_models.py:867-905: (estimates, their standard errors, total cost)"""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if mfmc_data is None:
            mfmc_data = self.setup_mfmc(budget=budget, eps=eps, continuous_relaxation=continuous_relaxation)
        best_group = list(mfmc_data["models"])
        samples = np.round(mfmc_data["samples"]).astype(np.int64)
        errs, tot_cost, alphas = mfmc_data["errors"], mfmc_data["total_cost"], mfmc_data["alphas"]
        if self.verbose: print("\nSampling optimal MFMC estimator...\n")
        L = len(best_group)
        y = [[0 for i in range(L)] for n in range(self.n_outputs)]
        y1 = [[0 for i in range(L - 1)] for n in range(self.n_outputs)]
        for i in range(L):
            N = samples[i]
            if i > 0: N -= samples[i - 1]
            sumse = self._group_sums(best_group[i:], N)
            for n in range(self.n_outputs):
                for j in range(i, L):
                    y[n][j] += sumse[n][j - i]
                    if j < L - 1: y1[n][j] += sumse[n][j - i + 1]
        for n in range(self.n_outputs):
            for i in range(L):
                y[n][i] /= samples[i]
                if i < L - 1: y1[n][i] /= samples[i]
        mu = [y[n][0] + sum(alphas[n][i] * (y[n][i + 1] - y1[n][i]) for i in range(L - 1)) for n in range(self.n_outputs)]
        return mu, errs, tot_cost

    def solve_mc(self, budget=None, eps=None):
        """bluest/blue_models.py:907-930: plain Monte Carlo on model 0"""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if eps is not None and np.isscalar(eps): eps = [eps for n in range(self.n_outputs)]
        Vs = np.array([self.get_covariance(n)[0, 0] for n in range(self.n_outputs)])
        cost = self.get_costs()[0]
        if budget is not None:
            N_MC = int(np.floor(budget / cost))
            errs = np.sqrt(np.maximum(Vs, 0.0) / N_MC)
            tot_cost = N_MC * cost
        else:
            N_MC = max(int(np.ceil(Vs[n] / eps[n]**2)) for n in range(self.n_outputs))
            tot_cost = N_MC * cost
            errs = np.sqrt(Vs / N_MC)
        if self.verbose: print("Standard MC estimator ready. Max error: ", max(errs), "Cost: ", tot_cost)
        if self.verbose: print("\nSampling standard MC estimator...\n")
        sumse = self._group_sums([0], N_MC)
        mu = [sumse[n][0] / N_MC for n in range(self.n_outputs)]
        return mu, errs, tot_cost

    # ---- SPD projection of the covariances (bluest/blue_models.py:348-433) ----------------------------------------------------
    def project_covariances(self, bypass_error_check=False):
        """bluest/blue_models.py:348-350; every output in one launch, then each handled in order as project_covariance(n)"""
        self._project(list(range(self.n_outputs)), bypass_error_check)

    def project_covariance(self, n=0, bypass_error_check=False):
        """bluest/blue_models.py:352-433: returns the projection error (the SPG objective, or ||C - C_new||_F when every entry
        is known)"""
        return self._project([n], bypass_error_check)[0]

    @in_host_section
    def _project(self, outputs, bypass_error_check):
        spg_params = self.params["spg_params"]
        if self.M > BLUEST_MAX_MODELS:
            raise BLUESTError("the SPD projection covers at most %d models (this problem has %d)" % (BLUEST_MAX_MODELS, self.M))
        Cs = [self.get_covariance(n) for n in outputs]
        results = None
        if self.mpiRank == 0:
            results = cov_project([np.where(np.isnan(C), 0.0, C) for C in Cs], [(~np.isnan(C)).astype(np.float64) for C in Cs],
                                  spg_params)
        results = self.comm.bcast(results, root=0)
        errs = []
        for n, C, (X, f, gpmax, it, count, info) in zip(outputs, Cs, results):
            finite = bool(np.isfinite(C).all())
            if info == BLUEST_COVPROJ_NONFINITE:
                raise BLUESTError("covariance %d has non-finite entries: it cannot be projected" % n)
            if finite:
                if info != 0:
                    raise BLUESTError("covariance %d: the eigendecomposition did not converge" % n)
                if self.verbose: print("Covariance projected to be symmetric positive definite, projection error: ", f)
                C_new = X
            else:
                if self.verbose: print("Running Spectral Gradient Descent for Covariance projection...")
                res = {"x": X.flatten(), "f": f, "gpmax": gpmax, "it": it, "count": count, "solver_info": info}
                if spg_params["verbose"] and self.warning:
                    self._print_spg_summary(res)
                if info == 0:
                    if self.verbose: print("Covariance projected, projection error: ", f)
                    if f > spg_params["eps"] and self.verbose and not bypass_error_check:
                        print("\n\n++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++")
                        print("\nWARNING! Large covariance projection error. Model covariance may be singular. Consider removing one model.")
                        print("Leaving covariances as they are. To bypass: run problem.project_variances(bypass_error_check=True) before setting up UQ solver.\n")
                        print("++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++++\n\n")
                        errs.append(f)
                        continue
                elif info in (BLUEST_COVPROJ_MAXIT, BLUEST_COVPROJ_MAXFEV):
                    raise RuntimeError("Could not find good enough Covariance projection. Solver info:\n%s" % res)
                else:
                    raise BLUESTError("covariance %d: the eigendecomposition did not converge" % n)
                C_new = X.copy()
                sd = np.sqrt(np.diag(C_new))
                rho_new = C_new / np.outer(sd, sd)
                C_new[abs(rho_new) < 1.0e-7] = 0.0              # uncorrelated (the reference marks them inf: covariance 0)
            self._coupling[n].update(C_new)
            errs.append(f)
        return errs

    @staticmethod
    def _print_spg_summary(res):
        """the closing report of bluest/spg.py:105-132 (the per-iteration lines are not kept on the device)"""
        print("\nSPECTRAL PROJECTED GRADIENT METHOD.\n")
        print("Problem size:\t%d\n" % len(res["x"]))
        print(" %d\t %e\t %e" % (res["it"], res["f"], res["gpmax"]))
        print("\n")
        print("Number of iterations               : %d\n" % res["it"])
        print("Number of functional evaluations   : %d\n" % res["count"])
        print("Objective function value           : %e\n" % res["f"])
        print("Sup-norm of the projected gradient : %e\n" % res["gpmax"])
        if res["solver_info"] == 0:
            print("SPG: Optimal solution found.\n")
        elif res["solver_info"] == 1:
            print("WARNING! SPG: Maximum number of iterations reached.\n")
        else:
            print("WARNING! SPG: Maximum number of functional evaluations reached.\n")

    # ---- refused ----------------------------------------------------------------------------------------------------------------
    def _out_of_scope(self, *a, **k):
        raise BLUESTError("outside this GPU build (SURVEY.md section 2): only setup_solver() / solve(), setup_mfmc() / solve_mfmc() "
                          "and solve_mc() with given covariances")

    setup_mlmc = solve_mlmc = setup_mc = _out_of_scope
    save_graph_data = load_graph_data = estimate_missing_covariances = estimate_costs = _out_of_scope
    complexity_test = variance_test = _out_of_scope

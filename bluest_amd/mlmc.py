"""
MLMCMixin -- the multilevel Monte Carlo estimator of bluest/blue_models.py:578-769 (setup_mlmc / solve_mlmc /
compute_mlmc_data, with the reference's signatures and return values) for a BLUEProblem:

    class MyProblem(MLMCMixin, BLUEProblem):
        def sampler(self, ls, N=1): ...
        def evaluate(self, ls, samples, N=1): ...

BLUEProblem itself refuses setup_mlmc / solve_mlmc; the mix-in, listed first, provides them.

setup_mlmc takes the argmin over every group of models through model 0, ordered by decreasing cost, whose consecutive models
are coupled in the intersection of the coupling graphs.  The search runs on the GPU (bluest_mlmc_search, csrc/mlmc.hip); the
host orders the models, fills the table of level variances, and finishes the winner as blue_models.py:725-734 does.

Differences from the reference, both where it fails without a message:
  - no admissible group is feasible: BLUESTError (the reference dies with a KeyError on its empty best_data);
  - solve_mlmc on an estimator whose budget adjustment left a level without samples: BLUESTError (the reference divides by
    zero).
A quirk of the reference kept on purpose (:718): with a tolerance, groups are compared by the samples times the MODEL costs
w[g_i], not the level costs w[g_i] + w[g_i+1] that total_cost of attempt_mlmc_setup uses.
Limits: at most 30 models below model 0 in cost order (2^30 subsets); the integer rounding covers groups of at most 24 models
('Too many dimensions to brute-force it' beyond, as in the reference).
"""
import ctypes

import numpy as np

from . import _lib, misc
from .host import in_host_section
from .sap import BLUESTError

BLUEST_MLMC_MAX_CANDIDATES = 30      # include/bluest_hip.h, Part 9
BLUEST_MLMC_BUDGET, BLUEST_MLMC_CONTINUOUS = 1, 2
BLUEST_MLMC_NONE, BLUEST_MLMC_TOO_BIG = 1, 2

_SCALARS = (int, float, np.int64, np.float64, np.int32, np.float32)


class MLMCMixin(object):
    def _mlmc_order(self):
        """models by decreasing cost, the ones dearer than model 0 dropped (blue_models.py:652-658)"""
        lme = len(self.check_costs(warning=True))
        w = self.get_costs()
        idx = np.argsort(w)[::-1][lme:]
        if idx[0] != 0:
            raise BLUESTError("model 0 is not the first model in cost order (a model costs exactly as much): MLMC needs it first")
        return w, idx

    def _mlmc_warn(self, dV):
        # this is only True if all dVn are entirely populated with NaNs/infs
        if not any(np.isfinite(dVn).any() for dVn in dV):
            if self.mpiRank == 0: print("\nWarning! MLMC variances were not provided nor estimated. The resulting MLMC estimator might be suboptimal.\n")

    def _mlmc_linked(self):
        return np.logical_and.reduce([cp.linked for cp in self._coupling])      # nx.intersection_all(self.G)

    def compute_mlmc_data(self, group, samples):
        """bluest/blue_models.py:578-639: the MLMC estimator of `group` (model 0 first) with the given samples per level"""
        samples = np.array(samples)
        group = [int(g) for g in group]
        w, _ = self._mlmc_order()
        CC, dV = self.get_covariances(), self.get_mlmc_variances()
        linked = self._mlmc_linked()
        if not all(i != j and linked[i, j] for i, j in zip(group[:-1], group[1:])):
            raise ValueError("Group given is not compatible with MLMC.")
        if group[0] != 0:
            raise ValueError("The high-fidelity model, model 0, should be the first in the given group!")
        self._mlmc_warn(dV)
        errs, mlmc_costs = np.zeros((self.n_outputs,)), np.zeros((self.n_outputs,))
        for n in range(self.n_outputs):
            v, subw = misc.mlmc_levels(CC[n], dV[n], w, group)
            errs[n] = sum(v[samples > 0] / samples[samples > 0])
            mlmc_costs[n] = samples @ subw
        return {"models": group, "samples": samples, "errors": errs, "total_cost": max(mlmc_costs)}

    @in_host_section
    def setup_mlmc(self, budget=None, eps=None, continuous_relaxation=False):
        """bluest/blue_models.py:642-741: the best MLMC estimator over every admissible group through model 0, searched on the
        GPU (bluest_mlmc_search).  Returns {"models", "samples", "errors", "total_cost"}; samples are per level."""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if eps is not None and isinstance(eps, _SCALARS): eps = [eps for n in range(self.n_outputs)]
        if eps is None: eps = [None for n in range(self.n_outputs)]
        w, idx = self._mlmc_order()
        if self.verbose: print("Setting up optimal MLMC estimator...\n")
        if len(idx) - 1 > BLUEST_MLMC_MAX_CANDIDATES:
            raise BLUESTError("%d models below model 0 in cost order: the MLMC search covers at most %d (2^%d subsets)"
                              % (len(idx) - 1, BLUEST_MLMC_MAX_CANDIDATES, BLUEST_MLMC_MAX_CANDIDATES))
        CC, dV = self.get_covariances(), self.get_mlmc_variances()
        self._mlmc_warn(dV)
        data = None
        if self.mpiRank == 0:
            data = self._mlmc_search(CC, dV, w, idx, budget, eps, continuous_relaxation)
            if self.verbose: print("Best MLMC estimator found. Coupled models:", data["models"], " Max error: ", max(data["errors"]),
                                   " Cost: ", data["total_cost"], "\n")
        return self.comm.bcast(data, root=0)

    def _mlmc_search(self, CC, dV, w, idx, budget, eps, continuous_relaxation):
        linked = self._mlmc_linked()
        nb, n_out = len(idx) - 1, self.n_outputs
        lv = np.full((n_out, nb + 1, nb + 1), np.nan)
        for n in range(n_out):
            for p in range(nb + 1):
                lv[n, p, p] = CC[n][idx[p], idx[p]]
                for q in range(p + 1, nb + 1):
                    lv[n, p, q] = misc.mlmc_levels(CC[n], dV[n], w, [idx[p], idx[q]])[0][0]
        adj = np.array([sum(1 << q for q in range(nb + 1) if q != p and linked[idx[p], idx[q]]) for p in range(nb + 1)],
                       dtype=np.uint32)
        flags = (BLUEST_MLMC_BUDGET if budget is not None else 0) | (BLUEST_MLMC_CONTINUOUS if continuous_relaxation else 0)
        eps2 = None if budget is not None else np.array([e**2 for e in eps], dtype=np.float64)
        wl = np.ascontiguousarray(w[idx], dtype=np.float64)
        mask, obj, status = ctypes.c_uint32(0), ctypes.c_double(0.0), ctypes.c_int32(0)
        combo = np.zeros(n_out, dtype=np.uint32)
        _lib.check(_lib.lib().bluest_mlmc_search(nb, n_out, flags, float(budget or 0.0), _lib.ptr(eps2), _lib.ptr(wl), _lib.ptr(lv),
                                                 _lib.ptr(adj), ctypes.byref(mask), _lib.ptr(combo), ctypes.byref(obj),
                                                 ctypes.byref(status), None))
        if status.value == BLUEST_MLMC_TOO_BIG:
            raise ValueError('Too many dimensions to brute-force it')
        if status.value != 0:
            raise BLUESTError("no group of models admits an MLMC estimator")
        group = [int(idx[p]) for p in range(nb + 1) if p == 0 or (mask.value >> (p - 1)) & 1]
        # every output's samples on the chosen group, then the element-wise maximum per level (blue_models.py:725-734)
        per_output = []
        for n in range(n_out):
            v, subw = misc.mlmc_levels(CC[n], dV[n], w, group)
            m, variance = misc.mlmc_allocation(v, subw, budget=budget, eps=eps[n])
            if not continuous_relaxation:
                m = misc.mfmc_round_from_combo(m, combo[n])
            per_output.append((m, variance))
        samples = np.max(np.vstack([m for m, _ in per_output]), axis=0)
        wg = w[group]
        cost = samples @ wg
        if budget is not None:  # adjust if budget bound. The max above already takes care of the variance bound.
            samples = np.floor(samples - (max(cost - budget, 0) / (wg @ wg)) * wg).astype(int)
            samples[0] = max(samples[0], 1)  # need at least one sample on level 0
            cost = samples @ wg
        errs = [np.sqrt(variance(samples)) for _, variance in per_output]
        return {"models": group, "samples": samples, "errors": errs, "total_cost": cost}

    def solve_mlmc(self, budget=None, eps=None, mlmc_data=None):
        """bluest/blue_models.py:743-769: (estimates, their standard errors, total cost)"""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if mlmc_data is None:
            mlmc_data = self.setup_mlmc(budget=budget, eps=eps, continuous_relaxation=False)
        best_group = list(mlmc_data["models"])
        samples = np.round(mlmc_data["samples"]).astype(np.int64)
        errs, tot_cost = mlmc_data["errors"], mlmc_data["total_cost"]
        if (samples <= 0).any():
            raise BLUESTError("a level of the MLMC estimator has no samples (%s on the groups of %s): the budget adjustment "
                              "removed them" % (samples.tolist(), best_group))
        if self.verbose: print("\nSampling optimal MLMC estimator...\n")
        L = len(best_group)
        groups = [list(item) for item in zip(best_group[:-1], best_group[1:])] + [[best_group[-1]]]
        mu = [0 for n in range(self.n_outputs)]
        for i in range(L):
            N = samples[i]
            sumse = self._group_sums(groups[i], N)
            for n in range(self.n_outputs):
                if i < L - 1: mu[n] += (sumse[n][0] - sumse[n][1]) / N
                else:         mu[n] += sumse[n][0] / N
        return mu, errs, tot_cost

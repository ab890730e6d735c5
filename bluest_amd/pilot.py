"""
Pilot samples -> covariances, MLMC difference variances and costs (bluest/blue_models.py:76-101, :265-299, :326-346, :435-441).

pilot_statistics(values)  the sums the estimates are made of, on the GPU (bluest_pilot_stats, csrc/pilot.hip): per output the sums
                          of y_i, of y_i y_j, and -- from the explicit differences -- of (y_i - y_j) and (y_i - y_j)^2.  The
                          result depends on the values and on BLUEST_PILOT_CHUNK only: the same bits on every run and machine.

PilotMixin                what BLUEProblem alone refuses, opt-in like bluest_amd.mlmc.MLMCMixin:

    class MyProblem(PilotMixin, BLUEProblem):
        def sampler(self, ls, N=1): ...
        def evaluate(self, ls, samples, N=1): ...

    MyProblem(M, n_outputs=2, costs=w, covariance_estimation_samples=32)          # C=None: everything is estimated
    MyProblem(M, C=C_with_NaN, ...)       # NaN = coupled, to be estimated; inf = never coupled; 0 = uncorrelated
    MyProblem(M, C=C)                     # costs=None: estimated from problem.cost, else from the time spent in evaluate
    p.save_graph_data("graph.npz");  MyProblem(M, datafile="graph.npz")           # the reference's file layout, both ways

The constructor follows the reference's order: coupling graphs from C, estimate_costs() if no costs were given,
estimate_missing_covariances(N) with N = params["covariance_estimation_samples"] (default 100) rounded up to a multiple of the
communicator size, then BLUEProblem's projection (unless skip_projection) and graph check.  The sampler is called exactly as the
reference's blue_fn calls it -- sampler(ls) when it takes one argument, else sampler(ls, N2) in batches of
params["sample_batch_size"]; with a batch size of 1 the model outputs are scalars, otherwise arrays of length N2; a batch with
a non-finite output is drawn again -- so a seeded sampler gives the samples it gives the reference.  All values are collected
into one [n_outputs, N, L] array and ONE pilot_statistics call follows.  A class that overrides get_models_inner_products has
inner products written in Python: the same flow then takes its sums from blue_fn(..., compute_mlmc_differences=True) on the
host.  With an MPI communicator each rank samples its share (the split of BLUEProblem._group_sums), rank 0 gathers the values,
runs the kernel and broadcasts the sums.

Differences from the reference:
  - it indexes the estimate C_hat, which covers only the models with an unknown entry, by the GLOBAL model numbers
    (blue_models.py:342-346), which is right only when every model has an unknown entry; here the estimate is read at the model's
    position among the sampled ones;
  - the arrays passed as mlmc_variances are copied, not written into;
  - the warning about a model dearer than model 0 is printed where BLUEProblem prints it, at the end of the constructor.
Still refused (BLUESTError): sample files (`samplefile`, `outputs_to_save`) and reorder_graph_nodes; complexity_test and variance_test
are refused by this mix-in alone and provided by bluest_amd.estimator.SamplingMixin.
"""
import ctypes

import numpy as np

from . import _lib
from ._blue_fn import blue_fn, draw_values
from .blue_models import BLUEProblem, _Coupling, BLUEST_MAX_MODELS
from .sap import BLUESTError

BLUEST_PILOT_CHUNK = 128             # include/bluest_hip.h, Part 10
BLUEST_PILOT_MAX_OUTPUTS = 1024
SLAB_BYTES = 256 << 20               # a host array larger than this goes to the GPU in slabs of whole chunks


def _stats_call(values, N, L, n_out, differences, stream):
    sumse, sumsc = np.empty((n_out, L)), np.empty((n_out, L, L))
    sumsd1 = np.empty((n_out, L, L)) if differences else None
    sumsd2 = np.empty((n_out, L, L)) if differences else None
    _lib.check(_lib.lib().bluest_pilot_stats(N, L, n_out, _lib.ptr(values), _lib.ptr(sumse), _lib.ptr(sumsc), _lib.ptr(sumsd1),
                                             _lib.ptr(sumsd2), stream))
    return sumse, sumsc, sumsd1, sumsd2


def pilot_statistics(values, differences=True, slab_bytes=SLAB_BYTES):
    """(sumse [n_out, L], sumsc [n_out, L, L], sumsd1, sumsd2 [n_out, L, L]) as numpy arrays from values[n, s, i] = output n of
    model i on sample s: a numpy array or a CUDA torch tensor of shape [n_out, N, L] (float64).  sumsd1 / sumsd2 hold the sums of
    y_i - y_j and (y_i - y_j)^2 at i < j and 0 elsewhere; they are None when `differences` is False.  A host array of more than
    `slab_bytes` is fed output by output in slabs of whole chunks of BLUEST_PILOT_CHUNK samples (of at most `slab_bytes`), and
    the slabs' sums are added in order: still a function of the values, BLUEST_PILOT_CHUNK and `slab_bytes` only."""
    if hasattr(values, "data_ptr"):                                     # a torch tensor
        import torch
        if values.dim() != 3 or values.dtype != torch.float64:
            raise ValueError("values must be a float64 array of shape [n_outputs, N, L]")
        if not values.is_cuda:
            values = values.numpy()
        else:
            values = values.contiguous()
            n_out, N, L = (int(d) for d in values.shape)
            with torch.cuda.device(values.device):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                return _stats_call(values, N, L, n_out, differences, stream)
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3:
        raise ValueError("values must be a float64 array of shape [n_outputs, N, L]")
    n_out, N, L = values.shape
    values = np.ascontiguousarray(values)
    if values.nbytes <= slab_bytes:
        return _stats_call(values, N, L, n_out, differences, None)
    # one output at a time: a run of samples of ONE output is contiguous as it lies, so no slab is repacked on the host
    per_slab = max(int(slab_bytes) // max(L * 8, 1) // BLUEST_PILOT_CHUNK, 1) * BLUEST_PILOT_CHUNK
    outputs = []
    for n in range(n_out):
        total = None
        for start in range(0, N, per_slab):
            slab = values[n:n + 1, start:start + per_slab, :]
            part = _stats_call(slab, slab.shape[1], L, 1, differences, None)
            total = part if total is None else tuple(None if t is None else t + q for t, q in zip(total, part))
        outputs.append(total)
    return tuple(None if parts[0] is None else np.concatenate(parts, axis=0) for parts in zip(*outputs))


def next_divisible_number(x, n):
    return n * (x // n + int(x % n > 0))


class PilotMixin(object):
    _unknown_ok = True
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message

    # ---- BLUEProblem's hooks ----------------------------------------------------------------------------------------------------
    def _init_inputs(self, C, costs):
        if self.params.get("samplefile") is not None or self.params.get("outputs_to_save") is not None:
            raise BLUESTError("sample files (samplefile, outputs_to_save) are outside this GPU build (SURVEY.md section 2)")
        if C is None:
            C = [np.nan * np.ones((self.M, self.M)) for n in range(self.n_outputs)]
        self._costs_given = costs is not None
        if costs is None:
            costs = np.nan * np.ones(self.M)
        return C, costs

    def _complete_inputs(self):
        self.dV = [np.array(d, dtype=np.float64) for d in self.dV]
        if not self._costs_given:
            self.estimate_costs(self.get_comm().Get_size())
        self.estimate_missing_covariances(next_divisible_number(int(self.params.get("covariance_estimation_samples", 100)),
                                                                self.mpiSize))
        if self.params["skip_projection"]:           # otherwise BLUEProblem checks the graphs after its projection
            for cp in self._coupling:
                cp.check(self.params["remove_uncorrelated"])

    def _init_from_datafile(self, datafile, costs):
        self.load_graph_data(datafile, costs)
        self.check_costs(warning=True)
        if self.verbose: print("\nBLUE estimator ready.\n")

    # ---- sampling -----------------------------------------------------------------------------------------------------------------
    def blue_fn(self, ls, N, verbose=True, compute_mlmc_differences=False):
        """bluest/blue_models.py:445-446"""
        return blue_fn(ls, N, self, sampler=self.sampler, inners=self.get_models_inner_products(), comm=self.get_comm(),
                       N1=self.params["sample_batch_size"], No=self.n_outputs, compute_mlmc_differences=compute_mlmc_differences,
                       verbose=self.verbose and verbose)

    def outer(self, a, b, inner):
        """bluest/blue_models.py:186-196"""
        L = len(a)
        out = np.zeros((L, L))
        for i in range(L):
            for j in range(L):
                out[i, j] = inner(a[i], b[j])
        return out

    def _pilot_values(self, ls, N):
        """this rank's share of N joint samples of the models `ls` as an array [n_outputs, share, len(ls)], drawn with the
        reference's sequence of sampler / evaluate calls (bluest/blue_fn.py:106-129)"""
        return draw_values(self, ls, N)

    def _pilot_gathered(self, ls, values):
        """rank 0: the values of all ranks [n_outputs, N, len(ls)] on their way to pilot_statistics.  Nothing to do here;
        bluest_amd.pilot_errors.PilotErrorsMixin keeps them"""
        return values

    def _pilot_sums(self, ls, N):
        """per output sumse [L], sumsc [L, L], sumsd1, sumsd2 [L, L] (i < j) over N joint samples of the models `ls`"""
        if type(self).get_models_inner_products is not BLUEProblem.get_models_inner_products:
            sumse, sumsc, _, sumsd1, sumsd2 = self.blue_fn(ls, N, compute_mlmc_differences=True)
            return sumse, sumsc, sumsd1, sumsd2
        if len(ls) > BLUEST_MAX_MODELS or self.n_outputs > BLUEST_PILOT_MAX_OUTPUTS:
            raise BLUESTError("the pilot statistics cover at most %d models and %d outputs" % (BLUEST_MAX_MODELS, BLUEST_PILOT_MAX_OUTPUTS))
        comm = self.get_comm()
        parts = comm.gather(self._pilot_values(ls, N), root=0)
        sums = None
        if comm.Get_rank() == 0:                                        # the kernel runs on one rank, as the projection does
            values = self._pilot_gathered(ls, parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1))
            sums = pilot_statistics(values, differences=True)
        return comm.bcast(sums, root=0)

    # ---- estimators ---------------------------------------------------------------------------------------------------------------
    def estimate_costs(self, N=1):
        """bluest/blue_models.py:435-441: per model, one call that is thrown away and one that counts; the cost of a sample is
        problem.cost when the problem states one, else the time spent in evaluate"""
        if self.verbose: print("Cost estimation via sampling...")
        for l in range(self.M):
            self.blue_fn([l], self.get_comm().Get_size(), verbose=False)
            _, _, cost = self.blue_fn([l], N, verbose=False)
            self._costs[l] = cost / N

    def estimate_missing_covariances(self, N):
        """bluest/blue_models.py:326-346: sample jointly the models of every row with an unknown (NaN) covariance in any output,
        write the estimate to the unknown entries of coupled pairs (0 = uncorrelated where |rho| < 1e-7) and the variance of
        every difference to the entries of mlmc_variances that are not finite.  Nothing is sampled when nothing is unknown."""
        unknown = [cp.linked & np.isnan(cp.cov) for cp in self._coupling]
        ls = [int(l) for l in np.flatnonzero(np.logical_or.reduce(unknown).any(axis=1))]
        if len(ls) == 0: return
        N = int(N)
        if self.verbose: print("Covariance estimation with %d samples..." % N)
        sumse, sumsc, sumsd1, sumsd2 = self._pilot_sums(ls, N)
        inners = self.get_models_inner_products()
        if isinstance(sumse, np.ndarray):
            C_hat = [sumsc[n] / N - np.outer(sumse[n], sumse[n]) / N**2 for n in range(self.n_outputs)]
        else:
            C_hat = [sumsc[n] / N - self.outer(sumse[n], sumse[n], inners[n]) / N**2 for n in range(self.n_outputs)]
        self.dV = [np.array(d, dtype=np.float64) for d in self.dV]
        for n in range(self.n_outputs):
            for i in range(len(ls)):
                for j in range(i + 1, len(ls)):
                    if not np.isfinite(self.dV[n][ls[i], ls[j]]):
                        self.dV[n][ls[i], ls[j]] = sumsd2[n][i][j] / N - inners[n](sumsd1[n][i][j] / N, sumsd1[n][i][j] / N)
        where = {l: i for i, l in enumerate(ls)}
        for n, cp in enumerate(self._coupling):
            for gi, gj in zip(*np.nonzero(np.triu(unknown[n]))):
                i, j = where[int(gi)], where[int(gj)]
                c = C_hat[n][i, j]
                if abs(c / np.sqrt(C_hat[n][i, i] * C_hat[n][j, j])) < 1.0e-7:
                    c = 0.0                                             # uncorrelated (the reference marks it inf: covariance 0)
                cp.cov[gi, gj] = cp.cov[gj, gi] = c

    # ---- model-graph files (bluest/blue_models.py:265-299) --------------------------------------------------------------------------
    def save_graph_data(self, filename):
        """M, n_outputs, costs, C0.. (per output: 0 = not coupled, inf = coupled and uncorrelated, else the covariance), SG, dV"""
        if len({len(sg) for sg in self.SG}) > 1:
            raise BLUESTError("the outputs' connected components have different sizes (%s): the file layout holds them as one "
                              "array" % [len(sg) for sg in self.SG])
        if self.mpiRank == 0:
            C_dict = {"C%d" % n: cp.adjacency() for n, cp in enumerate(self._coupling)}
            np.savez(filename, M=self.M, n_outputs=self.n_outputs, costs=self.get_costs(), **C_dict,
                     SG=np.array(self.SG, dtype=np.int64), dV=np.array(self.dV, dtype=np.float64))
        self.comm.barrier()

    def load_graph_data(self, filename, costs=None):
        """the first n_outputs outputs of the file; `costs` overrides the file's; no estimation, projection or graph check"""
        data = dict(np.load(filename)) if self.mpiRank == 0 else None
        data = self.comm.bcast(data, root=0)
        if self.M != int(data["M"]) or self.n_outputs > int(data["n_outputs"]):
            raise ValueError("Loaded data number of models and/or number of outputs mismatch with the user-given values")
        self.SG = data["SG"].tolist()[:self.n_outputs]
        self._coupling = [_Coupling.from_adjacency(data["C%d" % n], self.SG[n]) for n in range(self.n_outputs)]
        self._costs = np.array(data["costs"] if costs is None else costs, dtype=np.float64)
        if self._costs.shape != (self.M,):
            raise ValueError("costs must have one entry per model")
        dV = data.get("dV", None)
        if dV is None:
            self.dV = [np.nan * np.ones((self.M, self.M)) for n in range(self.n_outputs)]
        else:
            self.dV = [np.array(dV[n], dtype=np.float64) for n in range(self.n_outputs)]

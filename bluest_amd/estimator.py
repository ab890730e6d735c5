"""
Sampling an allocation in batches: the sums over the samples of every selected model group, the BLUE estimators made of them,
and the reference's two self-checks (bluest/blue_models.py:540-576, :932-978; the accumulation of bluest/blue_fn.py:159-167).

group_sums(values, weights=None, repeat_of=None)
    column sums of many ragged segments in ONE call on the GPU (bluest_group_sums, csrc/gsums.hip).  A segment is the
    [n_out, N_s, L_s] values of one model group (of one repeat): a numpy array or a CUDA float64 torch tensor, mixed freely;
    device tensors are read where they lie.  With `weights` [n_out, sum L_s] it also returns mu [R, n_out], the weighted sums
    per repeat.  The order of every addition is fixed (include/bluest_hip.h, Part 11): the sums of a segment depend on its
    values and on BLUEST_GSUM_CHUNK only -- the same bits alone or inside a batch, from host or device memory, on every machine.

SamplingMixin   opt-in like bluest_amd.pilot.PilotMixin and bluest_amd.mlmc.MLMCMixin:

    class MyProblem(SamplingMixin, BLUEProblem):            # or (SamplingMixin, PilotMixin, BLUEProblem), (.., MLMCMixin, ..)
        def sampler(self, ls, N=1): ...
        def evaluate(self, ls, samples, N=1): ...           # may return CUDA tensors: the values then never leave the device

    _group_sums(ls, N)    the sampler is called as the reference's blue_fn calls it (sampler(ls, N2) in batches of
                          params["sample_batch_size"], sampler(ls) when it takes one argument, a non-finite batch drawn again),
                          then one group_sums call; solve_mfmc, solve_mc and solve_mlmc go through it.
    solve(...)            all selected groups are drawn, then one group_sums call with the weights
                          w[o][g] = C_{o,g}^-1 R_g v_o (v_o = row 0 of the pseudo-inverse of output o's Phi, 0 for a group that
                          is not in output o's mapping): mus comes from the device, the variances from the same solve that
                          gives v_o.  Above SLAB_BYTES of values the calls are flushed and the parts of mu added in order.
    variance_test(...)    bluest/blue_models.py:944-978: N estimators of one allocation, drawn repeat by repeat in the reference's
                          order and summed in batches of repeats; returns (err_ex, err).
    complexity_test(...)  bluest/blue_models.py:932-942 with solver="spg": the reference hard-codes solver="cvxpy" there, a
                          third-party back-end this build does not ship; returns (tot_cost, rate).

A class that overrides get_models_inner_products has outputs that are not plain numbers: it takes BLUEProblem's host path
throughout.  With an MPI communicator every rank draws its share (the split of BLUEProblem._group_sums), rank 0 gathers the
values, runs the kernel and broadcasts the result.  Still refused (BLUESTError): sample files and reorder_graph_nodes.
"""
import ctypes

import numpy as np

from . import _lib
from ._blue_fn import draw_values
from .blue_models import BLUEProblem, BLUEST_MAX_MODELS
from .sap import BLUESTError, status_to_python

BLUEST_GSUM_CHUNK = 128              # include/bluest_hip.h, Part 11
BLUEST_GSUM_MAX_OUTPUTS = 1024
SLAB_BYTES = 256 << 20               # staging budget of one call, and the bytes of drawn values after which solve() flushes


def _is_gpu_tensor(v):
    return hasattr(v, "data_ptr") and bool(v.is_cuda)


def _segment_table(values, who):
    """what the sample-sum entry points take: (the segments as they are passed on -- contiguous float64 numpy arrays and CUDA
    tensors, kept alive by the caller --, n_out, counts, sizes, the table of their addresses, the stream of the first device
    tensor's device or None)"""
    if len(values) == 0:
        raise ValueError("%s needs at least one segment" % who)
    keep, stream = [], None
    for v in values:
        if hasattr(v, "data_ptr"):
            import torch
            if v.dim() != 3 or v.dtype != torch.float64:
                raise ValueError("every segment must be a float64 array of shape [n_outputs, N, L]")
            if v.is_cuda:
                v = v.contiguous()
                if stream is None:
                    with torch.cuda.device(v.device):
                        stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
            else:
                v = v.numpy()
        if not _is_gpu_tensor(v):
            v = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
            if v.ndim != 3:
                raise ValueError("every segment must be a float64 array of shape [n_outputs, N, L]")
        keep.append(v)
    n_out = int(keep[0].shape[0])
    if any(int(v.shape[0]) != n_out for v in keep):
        raise ValueError("every segment must have the same number of outputs")
    counts = np.array([int(v.shape[1]) for v in keep], dtype=np.int64)
    sizes = np.array([int(v.shape[2]) for v in keep], dtype=np.int32)
    ptrs = (ctypes.c_void_p * len(keep))(*[_lib.ptr(v) if v.shape[1] > 0 else None for v in keep])
    return keep, n_out, counts, sizes, ptrs, stream


def group_sums(values, weights=None, repeat_of=None, R=None, slab_bytes=SLAB_BYTES):
    """sums: list over the segments of [n_out, L_s] numpy arrays, sums[s][n, j] = sum_i values[s][n, i, j]; with `weights`
    ([n_out, sum of L_s]) also mu [R, n_out], mu[r, n] = sum over the segments with repeat_of[s] == r of weights . sums
    (repeat_of: non-decreasing, default all 0; R: default repeat_of[-1] + 1).  `slab_bytes`: host segments go to the GPU in
    slabs of whole chunks of at most this size; the result does not depend on it."""
    keep, n_out, counts, sizes, ptrs, stream = _segment_table(values, "group_sums")
    S = len(keep)
    T = int(sizes.sum())
    sums = np.empty((n_out, T))
    mu = None
    if weights is not None:
        weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
        if weights.shape != (n_out, T):
            raise ValueError("weights must have shape [n_outputs, sum of the segments' sizes] = [%d, %d]" % (n_out, T))
        repeat_of = np.zeros(S, dtype=np.int64) if repeat_of is None else np.ascontiguousarray(np.asarray(repeat_of, dtype=np.int64))
        if repeat_of.shape != (S,):
            raise ValueError("repeat_of must have one entry per segment")
        R = int(repeat_of[-1]) + 1 if R is None else int(R)
        mu = np.empty((max(R, 0), n_out))
    with _lib.staging_budget(slab_bytes):
        _lib.check(_lib.lib().bluest_group_sums(S, n_out, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                                _lib.ptr(weights), int(R or 0), _lib.ptr(repeat_of) if weights is not None else None,
                                                _lib.ptr(sums), _lib.ptr(mu), stream))
    ends = np.cumsum(sizes)
    out = [sums[:, e - l:e].copy() for e, l in zip(ends.tolist(), sizes.tolist())]
    return out if weights is None else (out, mu)


def sampled_columns(out):
    """the sampled groups of the allocation `out` (a MOSAP_output) in the order of the group list: [(g, models, first column, m_g)],
    the first column counted over the columns of the sampled groups, as SamplingMixin._blue_weights() lays out W"""
    samples = np.asarray(out["samples"])
    cols, c = [], 0
    for g in np.flatnonzero(samples > 0).tolist():
        ls = [int(l) for l in out["flattened_groups"][g]]
        cols.append((g, ls, c, int(samples[g])))
        c += len(ls)
    return cols


def flushed_draws(problem, n_rep, cols, slab_bytes, draw, flush):
    """the draw / flush loop of every _sample_estimators: per repeat each of the sampled groups `cols` (sampled_columns) is drawn
    in the order of the group list, share, nbytes = draw(col): this rank's values as they go to the gather, and the bytes the
    group counts for over all ranks (so that every rank flushes at the same points).  Once `slab_bytes` are pending, and at the
    end, the shares are gathered and rank 0 calls flush(pending, shares): pending[i] = (repeat, col), shares[rank][i].  A flush
    never splits a group; it may begin or end inside a repeat."""
    comm = problem.get_comm()
    pending = []                                                        # (repeat, col, this rank's share)

    def flush_pending():
        if pending:
            shares = comm.gather([p[2] for p in pending], root=0)      # [rank][segment]
            if comm.Get_rank() == 0:
                flush([p[:2] for p in pending], shares)
            del pending[:]

    held = 0
    for r in range(n_rep):
        for col in cols:
            share, nbytes = draw(col)
            pending.append((r, col, share))
            held += nbytes
            if held >= slab_bytes:
                flush_pending()
                held = 0
    flush_pending()


def collecting_solve(problem, solve, attribute, empty, args):
    """(solve(**args), what the flush hooks filed meanwhile): `attribute` of the problem is `empty` while the solve runs and None
    again afterwards, whatever happens; what rank 0 collected is broadcast"""
    setattr(problem, attribute, empty)
    try:
        result = solve(**args)
        taken = getattr(problem, attribute)
    finally:
        setattr(problem, attribute, None)
    comm = problem.get_comm()
    return result, comm.bcast(taken if comm.Get_rank() == 0 else None, root=0)


def sampled_errors(problem, source, sampled, share, promised=True):
    """[n_outputs]: sqrt(sum_g m_g share(moments, n, g, ls, w)) over the sampled groups g of every output n whose BLUE weights w of
    the group's columns are not all zero; moments = sampled() is what the last solve() collected (it raises where there is
    nothing).  source="model" gives sqrt(Vs) of solve() again -- with `promised` straight from _blue_weights(), else from the
    same sum.  Rank 0 computes, every rank returns."""
    if source not in ("samples", "model"):
        raise ValueError("source must be 'samples' or 'model'")
    moments = sampled()
    comm = problem.get_comm()
    errs = None
    if comm.Get_rank() == 0:
        W, Vs = problem._blue_weights()
        if source == "model" and promised:
            errs = np.sqrt(np.asarray(Vs, dtype=np.float64))
        else:
            var = np.zeros(problem.n_outputs)
            for g, ls, c, m in sampled_columns(problem.MOSAP_output):
                for n in range(problem.n_outputs):
                    w = W[n, c:c + len(ls)]
                    if not w.any():                                     # the group is not in this output's mapping
                        continue
                    var[n] += m * share(moments, n, g, ls, w)
            errs = np.sqrt(var)
    return comm.bcast(errs, root=0)


class SamplingMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message

    def _host_outputs(self):
        """inner products written in Python: the outputs are not plain numbers, the sums stay on the host"""
        return type(self).get_models_inner_products is not BLUEProblem.get_models_inner_products

    def _check_width(self, L):
        if L > BLUEST_MAX_MODELS or self.n_outputs > BLUEST_GSUM_MAX_OUTPUTS:
            raise BLUESTError("group sums cover at most %d models per group and %d outputs" % (BLUEST_MAX_MODELS, BLUEST_GSUM_MAX_OUTPUTS))

    @staticmethod
    def _joined(parts):
        """the ranks' shares of one segment, in rank order"""
        parts = [p.cpu().numpy() if hasattr(p, "data_ptr") and len(parts) > 1 else p for p in parts]
        return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=1)

    # ---- one group ----------------------------------------------------------------------------------------------------------------
    def _group_sums(self, ls, N):
        """sum over N joint samples of the models `ls`, per output: [n_outputs][len(ls)] (what bluest/blue_fn.py returns first),
        from one group_sums call over values drawn with the reference's call sequence"""
        if self._host_outputs():
            return BLUEProblem._group_sums(self, ls, N)
        self._check_width(len(ls))
        if int(N) == 0:
            return [[0.0] * len(ls) for _ in range(self.n_outputs)]
        comm = self.get_comm()
        mine = draw_values(self, ls, N, device_ok=True)
        parts = comm.gather(mine if comm.Get_size() == 1 or not hasattr(mine, "data_ptr") else mine.cpu().numpy(), root=0)
        sums = None
        if comm.Get_rank() == 0:
            sums = [[float(x) for x in row] for row in group_sums([self._joined(parts)])[0]]
        return comm.bcast(sums, root=0)

    # ---- whole estimators ---------------------------------------------------------------------------------------------------------
    def _blue_weights(self):
        """rank 0: (W, Vs) for the current allocation -- the weights W [n_outputs, T] over the columns of the sampled groups in the
        order of the group list, mu_o = W[o] . sums, and the estimators' variances.  Computed once per allocation."""
        out = self.MOSAP_output
        cached = self.__dict__.get("_blue_weights_cache")
        if cached is not None and cached[0] is out:
            return cached[1]
        mos = self.MOSAP
        samples = np.asarray(out["samples"])
        cols = sampled_columns(out)
        col0 = {g: c for g, _, c, _ in cols}
        W, Vs = np.zeros((self.n_outputs, sum(len(ls) for _, ls, _, _ in cols))), []
        for n in range(self.n_outputs):
            sap, mp = mos.SAPS[n], np.asarray(mos.mappings[n])
            m = samples[mp].astype(np.float64)
            var, v, status = sap.plan.solve(sap.plan.phi(m))
            status_to_python(int(status[0, 0]), "compute_BLUE_estimator")
            v = v[0, 0].cpu().numpy()
            Vs.append(float(var[0, 0]))
            for k in range(1, sap.K + 1):
                lo, hi = int(sap.cumsizes[k - 1]), int(sap.cumsizes[k])
                hit = np.flatnonzero(m[lo:hi] != 0)
                if len(hit) == 0:
                    continue
                members = np.asarray(sap.groups[k - 1])[hit]                                   # (h, k) model numbers
                blocks = np.asarray(sap.invcovs[k - 1]).reshape(-1, k, k)[hit]                # (h, k, k) = C_g^-1
                w = np.einsum("hjs,hj->hs", blocks, v[members])
                for row, i in zip(w, hit.tolist()):
                    c = col0[int(mp[lo + i])]
                    W[n, c:c + k] = row
        result = (W, np.array(Vs))
        self._blue_weights_cache = (out, result)
        return result

    def _segments_flushed(self, where, segments):
        """rank 0, once per flush of _sample_estimators, before the segments are summed: where[i] = (repeat, number of the group
        in the group list) of segments[i] [n_outputs, N, L], all ranks' shares joined.  A flush never splits a segment.  Nothing is
        done with them here; bluest_amd.moments.MomentsMixin takes their second moments."""

    def _sample_estimators(self, n_rep):
        """mus [n_rep, n_outputs] of n_rep independent estimators of the current allocation: per repeat every selected group is
        drawn in the order of the group list; the segments are summed in group_sums calls of up to SLAB_BYTES of values (counted
        over all ranks, so that every rank flushes at the same points), the parts of mu added in order."""
        comm = self.get_comm()
        rank = comm.Get_rank()
        cols = sampled_columns(self.MOSAP_output)
        for _, ls, _, _ in cols:
            self._check_width(len(ls))
        W = self._blue_weights()[0] if rank == 0 else None
        mus = np.zeros((n_rep, self.n_outputs))

        def draw(col):
            _, ls, _, m = col
            mine = draw_values(self, ls, m, device_ok=True)
            if comm.Get_size() > 1 and hasattr(mine, "data_ptr"):
                mine = mine.cpu().numpy()
            return mine, m * len(ls) * self.n_outputs * 8

        def flush(pending, shares):
            first, last = pending[0][0], pending[-1][0]
            # every segment brings the weights of its own group
            weights = np.concatenate([W[:, c:c + len(ls)] for _, (_, ls, c, _) in pending], axis=1)
            joined = [self._joined([share[i] for share in shares]) for i in range(len(pending))]
            self._segments_flushed([(r, col[0]) for r, col in pending], joined)
            _, part = group_sums(joined, weights=weights, repeat_of=[r - first for r, _ in pending], R=last - first + 1)
            mus[first:last + 1] += part

        flushed_draws(self, n_rep, cols, SLAB_BYTES, draw, flush)
        return comm.bcast(mus if rank == 0 else None, root=0)

    def solve(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, verbose=True, continuous_relaxation=False,
              max_model_samples=None, optimization_solver_params=None):
        """bluest/blue_models.py:540-576: returns (estimates, their standard errors, total cost)"""
        if self._host_outputs():
            return BLUEProblem.solve(self, K=K, budget=budget, eps=eps, groups=groups, multi_groups=multi_groups, solver=solver,
                                     verbose=verbose, continuous_relaxation=continuous_relaxation,
                                     max_model_samples=max_model_samples, optimization_solver_params=optimization_solver_params)
        have = self.MOSAP_output
        changed = have is not None and ((budget is not None and budget != have["budget"]) or
                                        (eps is not None and np.any(np.asarray(eps) != np.asarray(have["eps"]))))
        if have is None or changed:
            self.setup_solver(K=K, budget=budget, eps=eps, groups=groups, multi_groups=multi_groups, solver=solver,
                              continuous_relaxation=continuous_relaxation, max_model_samples=max_model_samples,
                              optimization_solver_params=optimization_solver_params)
        if self.verbose and verbose: print("\nSampling BLUE...\n")
        mus = self._sample_estimators(1)[0]
        Vs = self.comm.bcast(self._blue_weights()[1] if self.mpiRank == 0 else None, root=0)
        return [float(x) for x in mus], np.sqrt(Vs), self.MOSAP_output["cost"]

    def variance_test(self, budget=None, eps=None, K=3, N=50, **kwargs):
        """bluest/blue_models.py:944-978: N estimators of one allocation; returns (err_ex, err), the error the allocation
        promises and the standard deviation of the N estimates, sqrt(s2 / N - s1^2 / N^2)"""
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if eps is not None and np.isscalar(eps): eps = [eps for n in range(self.n_outputs)]
        if self.verbose: print("Running variance test...", flush=True)
        self.setup_solver(K=K, budget=budget, eps=eps, **kwargs)
        err_ex = np.sqrt(self.MOSAP_output["variances"])
        err = np.zeros_like(err_ex)
        kwargs.pop("verbose", None)
        if self._host_outputs():
            inners = self.get_models_inner_products()
            s1, s2 = [0 for n in range(self.n_outputs)], np.zeros_like(err_ex)
            for it in range(1, N + 1):
                mus, _, _ = self.solve(K=K, budget=budget, eps=eps, verbose=False, **kwargs)
                for n in range(self.n_outputs):
                    s1[n] += mus[n]
                    s2[n] += inners[n](mus[n], mus[n])
            s1 = [inners[n](s1[n], s1[n]) for n in range(self.n_outputs)]
        else:
            mus = self._sample_estimators(int(N))
            s1, s2 = np.zeros(self.n_outputs), np.zeros(self.n_outputs)
            for it in range(int(N)):                                    # the reference's order of additions
                s1 += mus[it]
                s2 += mus[it] * mus[it]
            s1 = s1 * s1
        for n in range(self.n_outputs):
            err[n] = np.sqrt(s2[n] / N - s1[n] / N**2)
        if self.verbose: print("Theoretical error: ", err_ex, flush=True)
        if self.verbose: print("Estimated error:   ", err, flush=True)
        return err_ex, err

    def complexity_test(self, eps, K=3):
        """bluest/blue_models.py:932-942: the total cost of the allocation for every tolerance in `eps` and the slope of
        log2(cost) over the position in the list (2 when eps halves and cost ~ eps^-2).  The reference hard-codes
        solver="cvxpy" here, a third-party back-end this build does not ship: the allocations come from solver="spg"."""
        if self.verbose: print("Running cost complexity test...")
        tot_cost = []
        for i in range(len(eps)):
            self.setup_solver(K=K, eps=eps[i], solver="spg")
            tot_cost.append(self.MOSAP_output["cost"])
        tot_cost = np.array(tot_cost)
        rate = np.polyfit(np.arange(len(tot_cost)), np.log2(tot_cost), 1)[0]
        if self.verbose: print("Total costs   :", tot_cost)
        if self.verbose: print("Estimated rate:", rate)
        return tot_cost, rate

"""
blue_fn -- sample a group of coupled models and return the sums the BLUE estimator is made of (role of bluest/blue_fn.py:36-211,
exported by the reference's package next to SAP / MOSAP / BLUEProblem, bluest/__init__.py:7-10).

Host Python around the user's model: nothing here is on the accelerated path (SURVEY.md section 2 lists sampling as out of scope),
so this is the plain accumulation -- sums of the outputs and of their pairwise inner products, cost = evaluation time unless the
problem states its own -- with the reference's argument names.  With `compute_mlmc_differences=True` it also returns the sums
of the differences y_i - y_j and of their inner products with themselves (i < j), formed from the explicit differences as
blue_fn.py:147-157 forms them: the 5-tuple the covariance estimation of bluest_amd.pilot.PilotMixin takes when the problem
overrides `get_models_inner_products` (inner products written in Python cannot run on the GPU; for scalar outputs the mix-in
uses the kernel behind bluest_amd.pilot.pilot_statistics instead).  The sample files (`filename`, `outputs_to_save`) stay
refused.

draw_values -- the drawing loop alone (the reference's sequence of sampler / evaluate calls, blue_fn.py:106-129) without any
accumulation: the values go to the GPU in one piece (bluest_amd.pilot.PilotMixin, bluest_amd.estimator.SamplingMixin).
"""
import time
from inspect import signature

import numpy as np


class _Solo(object):
    """the communicator of a run without MPI"""

    def Get_rank(self): return 0
    def Get_size(self): return 1
    def allreduce(self, v, op=None): return v


def _all_finite(values):
    return all(bool(np.all(np.isfinite(v))) for out in values for v in out)


def _on_gpu(v):
    return hasattr(v, "is_cuda") and bool(v.is_cuda)


def draw_values(problem, ls, N, device_ok=False):
    """this rank's share of N joint samples of the models `ls` as an array [n_outputs, share, len(ls)], drawn with the
    reference's sequence of sampler / evaluate calls (bluest/blue_fn.py:106-129): the share is N // size, one more on the first
    N % size ranks; sampler(ls) when the sampler takes one argument, else sampler(ls, N2) in batches of
    params["sample_batch_size"]; a batch with a non-finite output is drawn again.  The one drawing loop of
    bluest_amd.pilot.PilotMixin and bluest_amd.estimator.SamplingMixin.  With `device_ok`, an evaluate that returns CUDA tensors
    keeps its batches on the device: the finite check is one torch.isfinite(...).all() and the result is a CUDA tensor."""
    from .sap import BLUESTError
    comm = problem.get_comm()
    size, rank = comm.Get_size(), comm.Get_rank()
    mine = int(N) // size + (1 if rank < int(N) % size else 0)
    batched = len(signature(problem.sampler).parameters) > 1
    N1 = int(problem.params["sample_batch_size"]) if batched else 1
    n_out, L = problem.n_outputs, len(ls)
    out = None
    batches = []                                                        # device batches [n_out, N2, L]
    done = 0
    while done < mine:
        N2 = min(N1, mine - done)
        while True:
            samples = problem.sampler(ls, N2) if batched else problem.sampler(ls)
            Ps = problem.evaluate(ls, samples)
            if device_ok and _on_gpu(Ps[0][0]):
                import torch
                cols = [[Ps[n][i].reshape(-1) for i in range(L)] for n in range(n_out)]
                for n in range(n_out):
                    for i in range(L):
                        if cols[n][i].numel() != N2:
                            raise BLUESTError("output %d of model %d has %d values for a batch of %d samples: non-scalar outputs "
                                              "need get_models_inner_products" % (n, ls[i], cols[n][i].numel(), N2))
                Ps = torch.stack([torch.stack(row, dim=1) for row in cols]).to(torch.float64)
                finite = bool(torch.isfinite(Ps).all())
            else:
                finite = _all_finite(Ps)
            if finite:
                break
            if problem.verbose:
                print("Warning! Problem evaluation returned inf or NaN value. Resampling...", flush=True)
        if _on_gpu(Ps):
            batches.append(Ps)
        else:
            if out is None:
                out = np.empty((n_out, mine, L))
            for n in range(n_out):
                for i in range(L):
                    v = np.asarray(Ps[n][i], dtype=np.float64)
                    if v.size != N2:
                        raise BLUESTError("output %d of model %d has %d values for a batch of %d samples: non-scalar outputs need "
                                          "get_models_inner_products" % (n, ls[i], v.size, N2))
                    out[n, done:done + N2, i] = v.reshape(N2)
        done += N2
    if batches:
        import torch
        if out is not None:
            raise BLUESTError("evaluate returned CUDA tensors for some batches and host values for others")
        return torch.cat(batches, dim=1).contiguous()
    return np.empty((n_out, mine, L)) if out is None else out


def blue_fn(ls, N, problem, sampler=None, inners=None, comm=None, N1=1, No=1, verbose=True, compute_mlmc_differences=False,
            filename=None, outputs_to_save=None):
    """(sumse, sumsc, cost), or (sumse, sumsc, cost, sumsd1, sumsd2) with compute_mlmc_differences: sumse[n][i] = sum over the N paths of output n of model ls[i], sumsc[n][i, j] = sum of the inner
    products of outputs i and j, cost = N * problem.cost if the problem states one, else the seconds spent in problem.evaluate;
    sumsd1[n][i][j], sumsd2[n][i][j], i < j: sums of d = (output of ls[i]) - (output of ls[j]) and of inners[n](d, d), 0 elsewhere.
    problem.evaluate(ls, samples) -> Ps[n][i]; sampler(ls) or sampler(ls, count) -> one input per model (default: the same
    standard normal draw for every model); with an MPI communicator the paths are split over its ranks and the sums reduced."""
    if filename is not None or outputs_to_save is not None:
        from .sap import BLUESTError
        raise BLUESTError("blue_fn: sample files are outside this GPU build (SURVEY.md section 2)")
    comm = comm if comm is not None else _Solo()
    rank, size = comm.Get_rank(), comm.Get_size()
    n_models = len(ls)
    if inners is None:
        inners = [lambda a, b: a * b] * No
    if sampler is None:
        rng = np.random.RandomState(1 + rank)

        def sampler(ls, count=1):
            draw = rng.randn(count)
            return [draw] * n_models
    batched = len(signature(sampler).parameters) > 1
    chunk = int(N1) if batched else 1
    todo = int(N) // size + (1 if rank < int(N) % size else 0)
    sumse = [[0] * n_models for _ in range(No)]
    sumsc = [np.zeros((n_models, n_models)) for _ in range(No)]
    if compute_mlmc_differences:
        sumsd1 = [[[0] * n_models for _ in range(n_models)] for _ in range(No)]
        sumsd2 = [[[0] * n_models for _ in range(n_models)] for _ in range(No)]
    spent = 0.0
    while todo > 0:
        count = min(chunk, todo)
        while True:                                        # a non-finite model output is drawn again
            inputs = sampler(ls, count) if batched else sampler(ls)
            t0 = time.time()
            Ps = problem.evaluate(ls, inputs)
            spent += time.time() - t0
            if _all_finite(Ps):
                break
            if verbose:
                print("blue_fn: non-finite model output for models %s, drawing again" % (ls,), flush=True)
        paths = (lambda v: [v]) if chunk == 1 else (lambda v: [v[q] for q in range(count)])
        for n in range(No):
            rows = [paths(Ps[n][i]) for i in range(n_models)]
            for i in range(n_models):
                for v in rows[i]:
                    sumse[n][i] = sumse[n][i] + v
            for i in range(n_models):
                for j in range(n_models):
                    sumsc[n][j, i] += np.sum([inners[n](a, b) for a, b in zip(rows[i], rows[j])])
            if compute_mlmc_differences:
                for i in range(n_models):
                    for j in range(i + 1, n_models):
                        for a, b in zip(rows[i], rows[j]):
                            sumsd1[n][i][j] = sumsd1[n][i][j] + (a - b)
                            sumsd2[n][i][j] = sumsd2[n][i][j] + inners[n](a - b, a - b)
        todo -= count
    cost = N * problem.cost if hasattr(problem, "cost") else comm.allreduce(spent)
    for n in range(No):
        sumsc[n] = comm.allreduce(sumsc[n])
        sumse[n] = [comm.allreduce(v) for v in sumse[n]]
        if compute_mlmc_differences:
            for i in range(n_models):
                for j in range(i + 1, n_models):
                    sumsd1[n][i][j] = comm.allreduce(sumsd1[n][i][j])
                    sumsd2[n][i][j] = comm.allreduce(sumsd2[n][i][j])
    if compute_mlmc_differences:
        return sumse, sumsc, cost, sumsd1, sumsd2
    return sumse, sumsc, cost

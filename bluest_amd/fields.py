"""
Outputs that are vectors ("fields") with a declared diagonal inner product <a, b> = sum_c w_c a_c b_c, on the GPU
(include/bluest_hip.h, Part 12; csrc/fields.hip).  The reference takes any Python callable from get_models_inner_products
(bluest/blue_models.py:117-119, examples/multi_output_example.py) and evaluates it once per pair and sample on the host; a
DECLARED weight vector -- w = 1 for `a @ b`, lumped-mass weights for a finite-element field -- can run on the device.

field_statistics(values, w, differences=True)
    values [N, L, d] (numpy or a CUDA float64 tensor, read in place), w [d] >= 0 -> (sumse [L, d], sumsc [L, L],
    sumsd1 [L, L, d], sumsd2 [L, L]): the sums of y_i, of <y_i, y_j>, and -- from the explicit differences, at i < j, else 0 --
    of y_i - y_j and <y_i - y_j, y_i - y_j>.  One output per call: outputs may differ in d.
field_group_sums(values, weights=None, repeat_of=None, R=None)
    values: list of [N_s, L_s, d] segments, host and device mixed -> sums (list of [L_s, d]) and, with weights [sum L_s],
    mu [R, d]: bluest_amd.estimator.group_sums for a field.
The order of every addition is fixed (Part 12): the same bits from host or device memory, alone or inside a batch, on every
machine; with d = 1 and w = 1 the bits of pilot_statistics and group_sums.  There is no CPU path.

FieldOutputsMixin   opt-in, listed first:

    class MyProblem(FieldOutputsMixin, SamplingMixin, PilotMixin, BLUEProblem):      # or with only one of the two
        def output_weights(self):  return [None, mass]      # per output: None = a number, or the d_n weights of a field
        def sampler(self, ls, N=1): ...
        def evaluate(self, ls, samples, N=1): ...           # Ps[n][i]: [d_n] (batch 1, one-argument sampler) or [N2, d_n]

    get_models_inner_products() is derived from output_weights(): a * b for a number, float(np.dot(a * w, b)) for a field, so
    every host formula that combines sums (outer, the dV line of estimate_missing_covariances, variance_test's s1 / s2) uses the
    inner product the kernels use.  The pilot sums, the group sums and the estimators then come from the two calls above, one
    call per output; a number is a field of one component (the same bits as without the mix-in).  The sampler is called exactly
    as the reference's blue_fn calls it, as in bluest_amd._blue_fn.draw_values.  solve() returns mus[n] as a float or an
    ndarray [d_n]; the variances come from the same solve as in SamplingMixin.  With an MPI communicator every rank draws its
    share, rank 0 gathers, runs the kernels and broadcasts.  Still refused: sample files and reorder_graph_nodes.
"""
import ctypes
from inspect import signature

import numpy as np

from . import _lib
from ._blue_fn import _all_finite, _on_gpu
from .blue_models import BLUEProblem, BLUEST_MAX_MODELS
from .estimator import SLAB_BYTES, SamplingMixin, flushed_draws, sampled_columns
from .sap import BLUESTError

BLUEST_FIELD_TILE = 8                # include/bluest_hip.h, Part 12


def _segment(v, what):
    """a [N, L, d] float64 segment as a contiguous numpy array or CUDA tensor"""
    if hasattr(v, "data_ptr"):
        import torch
        if v.dim() != 3 or v.dtype != torch.float64:
            raise ValueError("%s must be a float64 array of shape [N, L, d]" % what)
        if v.is_cuda:
            return v.contiguous()
        v = v.numpy()
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    if v.ndim != 3:
        raise ValueError("%s must be a float64 array of shape [N, L, d]" % what)
    return v


def _stream_of(v):
    import torch
    with torch.cuda.device(v.device):
        return ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)


def field_statistics(values, w, differences=True):
    """(sumse [L, d], sumsc [L, L], sumsd1 [L, L, d], sumsd2 [L, L]) as numpy arrays from values[s, i, c] = component c of model
    i on sample s and the weights w [d] of the inner product; sumsd1 / sumsd2 are None when `differences` is False"""
    values = _segment(values, "values")
    N, L, d = (int(x) for x in values.shape)
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    if w.shape != (d,):
        raise ValueError("w must have one weight per component: shape [%d]" % d)
    P = L * (L - 1) // 2
    sumse, sumsc = np.empty((L, d)), np.empty((L, L))
    flat = np.empty((max(P, 1), d)) if differences else None           # (never a null pointer for L = 1)
    sumsd2 = np.empty((L, L)) if differences else None
    stream = _stream_of(values) if hasattr(values, "data_ptr") else None
    _lib.check(_lib.lib().bluest_field_stats(N, L, d, _lib.ptr(values), _lib.ptr(w), _lib.ptr(sumse), _lib.ptr(sumsc),
                                             _lib.ptr(flat), _lib.ptr(sumsd2), stream))
    sumsd1 = None
    if differences:
        sumsd1 = np.zeros((L, L, d))
        iu = np.triu_indices(L, 1)                                      # row-major pairs i < j, the order of the ABI
        sumsd1[iu[0], iu[1]] = flat[:P]
    return sumse, sumsc, sumsd1, sumsd2


def _field_segment_table(values, who):
    """what the field entry points over ragged segments take: (the segments [N_s, L_s, d] as they are passed on -- contiguous
    float64 numpy arrays and CUDA tensors, kept alive by the caller --, d, counts, sizes, the table of their addresses, the stream
    of the first device tensor's device or None)"""
    if len(values) == 0:
        raise ValueError("%s needs at least one segment" % who)
    keep = [_segment(v, "every segment") for v in values]
    d = int(keep[0].shape[2])
    if any(int(v.shape[2]) != d for v in keep):
        raise ValueError("every segment must have the same number of components")
    stream = None
    for v in keep:
        if hasattr(v, "data_ptr"):
            stream = _stream_of(v)
            break
    counts = np.array([int(v.shape[0]) for v in keep], dtype=np.int64)
    sizes = np.array([int(v.shape[1]) for v in keep], dtype=np.int32)
    ptrs = (ctypes.c_void_p * len(keep))(*[_lib.ptr(v) if v.shape[0] > 0 else None for v in keep])
    return keep, d, counts, sizes, ptrs, stream


def field_group_sums(values, weights=None, repeat_of=None, R=None, slab_bytes=SLAB_BYTES):
    """sums: list over the segments of [L_s, d] numpy arrays, sums[s][j, c] = sum_i values[s][i, j, c]; with `weights`
    ([sum of L_s], one scalar per column) also mu [R, d], mu[r] = sum over the segments with repeat_of[s] == r of
    weights . sums (repeat_of: non-decreasing, default all 0; R: default repeat_of[-1] + 1).  `slab_bytes`: host segments go to
    the GPU in slabs of whole chunks of at most this size; the result does not depend on it."""
    keep, d, counts, sizes, ptrs, stream = _field_segment_table(values, "field_group_sums")
    S = len(keep)
    T = int(sizes.sum())
    sums = np.empty((T, d))
    mu = None
    if weights is not None:
        weights = np.ascontiguousarray(np.asarray(weights, dtype=np.float64))
        if weights.shape != (T,):
            raise ValueError("weights must have one entry per column: shape [%d]" % T)
        repeat_of = np.zeros(S, dtype=np.int64) if repeat_of is None else np.ascontiguousarray(np.asarray(repeat_of, dtype=np.int64))
        if repeat_of.shape != (S,):
            raise ValueError("repeat_of must have one entry per segment")
        R = int(repeat_of[-1]) + 1 if R is None else int(R)
        mu = np.empty((max(R, 0), d))
    with _lib.staging_budget(slab_bytes):
        _lib.check(_lib.lib().bluest_field_sums(S, d, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                                _lib.ptr(weights), int(R or 0), _lib.ptr(repeat_of) if weights is not None else None,
                                                _lib.ptr(sums), _lib.ptr(mu), stream))
    ends = np.cumsum(sizes)
    out = [sums[e - l:e].copy() for e, l in zip(ends.tolist(), sizes.tolist())]
    return out if weights is None else (out, mu)


def field_share(problem, N):
    """how many of N joint samples this rank draws"""
    comm = problem.get_comm()
    size, rank = comm.Get_size(), comm.Get_rank()
    return int(N) // size + (1 if rank < int(N) % size else 0)


def field_batches(problem, ls, N, widths, device_ok=False):
    """this rank's share of N joint samples of the models `ls`, one batch at a time: yields per batch the list over the outputs of
    [N2, len(ls), widths[n]], numpy arrays or -- with `device_ok`, where evaluate returns CUDA tensors -- CUDA float64 tensors.
    A batch is shaped, checked for finiteness, drawn again where a value is not finite, and mapped through _field_batch_hook
    before it is handed out; nothing of it is kept here once the next one is asked for.  The sampler / evaluate calls are those of
    draw_field_values, which is this generator with every batch kept."""
    mine = field_share(problem, N)
    batched = len(signature(problem.sampler).parameters) > 1
    N1 = int(problem.params["sample_batch_size"]) if batched else 1
    n_out, L = problem.n_outputs, len(ls)
    hook = getattr(problem, "_field_batch_hook", None)
    raw = hook(ls) if hook is not None else [None] * n_out

    def shaped(v, n, i, N2):
        d = widths[n] if raw[n] is None else raw[n][0][i]
        count = v.numel() if hasattr(v, "numel") else v.size
        last = v.shape[-1] if len(v.shape) > 0 else 1
        if count != N2 * d or (d > 1 and last != d):
            raise BLUESTError("output %d of model %d has shape %s for a batch of %d samples: %s declares %d "
                              "component(s)" % (n, ls[i], tuple(v.shape), N2, "output_weights()" if raw[n] is None else
                                                "output_operators()", d))
        return v.reshape(N2, d)

    done = 0
    while done < mine:
        N2 = min(N1, mine - done)
        while True:
            samples = problem.sampler(ls, N2) if batched else problem.sampler(ls)
            Ps = problem.evaluate(ls, samples)
            if device_ok and _on_gpu(Ps[0][0]):
                import torch
                Ps = [torch.stack([shaped(Ps[n][i], n, i, N2) for i in range(L)], dim=1).to(torch.float64) if raw[n] is None else
                      [shaped(Ps[n][i], n, i, N2).to(torch.float64) for i in range(L)] for n in range(n_out)]
                finite = all(bool(torch.isfinite(t).all()) for P in Ps for t in (P if isinstance(P, list) else [P]))
                if finite:
                    Ps = [raw[n][1](P) if isinstance(P, list) else P for n, P in enumerate(Ps)]
            else:
                finite = _all_finite(Ps)
            if finite:
                break
            if problem.verbose:
                print("Warning! Problem evaluation returned inf or NaN value. Resampling...", flush=True)
        if not _on_gpu(Ps[0]):
            batch = [np.empty((N2, L, widths[n])) for n in range(n_out)]
            for n in range(n_out):
                if raw[n] is not None:
                    batch[n][:] = raw[n][1]([shaped(np.asarray(Ps[n][i], dtype=np.float64), n, i, N2) for i in range(L)])
                    continue
                for i in range(L):
                    batch[n][:, i, :] = shaped(np.asarray(Ps[n][i], dtype=np.float64), n, i, N2)
            Ps = batch
            del batch
        done += N2
        samples = None
        yield Ps
        Ps = None                                                       # (the batch is the caller's alone from here on)


def draw_field_values(problem, ls, N, widths, device_ok=False):
    """this rank's share of N joint samples of the models `ls`, per output an array [share, len(ls), widths[n]]: the field-aware
    sibling of bluest_amd._blue_fn.draw_values, with the same sequence of sampler / evaluate calls (bluest/blue_fn.py:106-129).
    Ps[n][i] holds widths[n] components per sample: shape [d] for a batch of one, else [N2, d] (a number: N2 values).  With
    `device_ok`, an evaluate that returns CUDA tensors keeps its batches on the device.
    A problem may have a method _field_batch_hook(ls) (bluest_amd.field_maps.MappedFieldsMixin): it returns per output None, or
    (the widths of the models `ls` themselves, a function from their len(ls) raw batches [N2, d_i] to [N2, len(ls), widths[n]]).
    Such an output is checked for width and finiteness as it arrives and mapped, batch by batch, before it is kept."""
    mine = field_share(problem, N)
    n_out, L = problem.n_outputs, len(ls)
    out, batches, done = None, [], 0
    for Ps in field_batches(problem, ls, N, widths, device_ok=device_ok):
        if _on_gpu(Ps[0]):
            batches.append(Ps)
        else:
            if out is None:
                out = [np.empty((mine, L, widths[n])) for n in range(n_out)]
            N2 = Ps[0].shape[0]
            for n in range(n_out):
                out[n][done:done + N2] = Ps[n]
        done += int(Ps[0].shape[0])
    if batches:
        import torch
        if out is not None:
            raise BLUESTError("evaluate returned CUDA tensors for some batches and host values for others")
        return [torch.cat([b[n] for b in batches], dim=0).contiguous() for n in range(n_out)]
    return [np.empty((mine, L, widths[n])) for n in range(n_out)] if out is None else out


def _joined(parts):
    """the ranks' shares of one segment [share, L, d], in rank order"""
    parts = [p.cpu().numpy() if hasattr(p, "data_ptr") and len(parts) > 1 else p for p in parts]
    return parts[0] if len(parts) == 1 else np.concatenate(parts, axis=0)


class FieldOutputsMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message

    # ---- what the user declares -----------------------------------------------------------------------------------------------------
    def output_weights(self):
        """per output: None for a number, or the d_n non-negative weights w of the inner product sum_c w_c a_c b_c"""
        return [None] * self.n_outputs

    def _field_weights(self):
        """per output the weights as an array [d_n] (a number: [1.0]) and whether it is a field"""
        declared = list(self.output_weights())
        if len(declared) != self.n_outputs:
            raise BLUESTError("output_weights() must have one entry per output (%d), not %d" % (self.n_outputs, len(declared)))
        ws = []
        for n, w in enumerate(declared):
            w = np.ones(1) if w is None else np.array(w, dtype=np.float64)
            if w.ndim != 1 or w.size < 1 or not np.all(np.isfinite(w)) or np.any(w < 0):
                raise BLUESTError("output_weights()[%d] must be None or a 1-D array of finite weights >= 0" % n)
            ws.append(w)
        return ws, [w is not None for w in declared]

    def get_models_inner_products(self):
        ws, is_field = self._field_weights()
        return [(lambda a, b, w=w: float(np.dot(a * w, b))) if f else (lambda a, b: a * b) for w, f in zip(ws, is_field)]

    def _host_outputs(self):
        return False

    @staticmethod
    def _plain(row, is_field):
        """a row [d] of sums as the host formulas take it: the vector of a field, the float of a number"""
        return np.array(row) if is_field else float(row[0])

    def _check_field_width(self, L):
        if L > BLUEST_MAX_MODELS:
            raise BLUESTError("the field sums cover at most %d models per group" % BLUEST_MAX_MODELS)

    def _gathered(self, mine):
        """rank 0: per output the values of all ranks, [N, L, d_n]; None on the other ranks"""
        comm = self.get_comm()
        if comm.Get_size() > 1:
            mine = [v.cpu().numpy() if hasattr(v, "data_ptr") else v for v in mine]
        parts = comm.gather(mine, root=0)
        if comm.Get_rank() != 0:
            return None
        return [_joined([share[n] for share in parts]) for n in range(self.n_outputs)]

    # ---- pilot samples (bluest_amd.pilot.PilotMixin) ----------------------------------------------------------------------------------
    def _field_pilot_count(self, ls, N):
        """how many of the N joint pilot samples of the models `ls` are drawn now: all of them.
        bluest_amd.field_pilot_errors.FieldPilotErrorsMixin draws what its earlier rounds have not"""
        return N

    def _field_pilot_gathered(self, ls, values):
        """rank 0: per output the values just drawn, all ranks' shares joined [count, L, d_n]; returns the values to sum, per
        output [N, L, d_n].  Nothing to do here; FieldPilotErrorsMixin puts the values of its earlier rounds in front"""
        return values

    def _pilot_sums(self, ls, N):
        """blue_fn's nested results -- sumse[n][i], sumsc[n] [L, L], sumsd1[n][i][j], sumsd2[n][i][j] (i < j, else 0) -- from ONE
        field_statistics call per output over all the values"""
        self._check_field_width(len(ls))
        ws, is_field = self._field_weights()
        values = self._gathered(draw_field_values(self, ls, self._field_pilot_count(ls, N), [len(w) for w in ws], device_ok=True))
        sums = None
        if values is not None:
            values = self._field_pilot_gathered(ls, values)
            L = len(ls)
            sumse, sumsc, sumsd1, sumsd2 = [], [], [], []
            for n in range(self.n_outputs):
                se, sc, d1, d2 = field_statistics(values[n], ws[n], differences=True)
                sumse.append([self._plain(se[i], is_field[n]) for i in range(L)])
                sumsc.append(sc)
                sumsd1.append([[self._plain(d1[i, j], is_field[n]) if i < j else 0 for j in range(L)] for i in range(L)])
                sumsd2.append([[float(d2[i, j]) if i < j else 0 for j in range(L)] for i in range(L)])
            sums = (sumse, sumsc, sumsd1, sumsd2)
        return self.get_comm().bcast(sums, root=0)

    # ---- one group --------------------------------------------------------------------------------------------------------------------
    def _group_sums(self, ls, N):
        """sum over N joint samples of the models `ls`: [n_outputs][len(ls)], each a float or an ndarray [d_n], from one
        field_group_sums call per output"""
        self._check_field_width(len(ls))
        ws, is_field = self._field_weights()
        if int(N) == 0:
            return [[np.zeros(len(w)) if f else 0.0 for _ in ls] for w, f in zip(ws, is_field)]
        values = self._gathered(draw_field_values(self, ls, N, [len(w) for w in ws], device_ok=True))
        sums = None
        if values is not None:
            sums = []
            for n in range(self.n_outputs):
                got = field_group_sums([values[n]])[0]
                sums.append([self._plain(got[i], is_field[n]) for i in range(len(ls))])
        return self.get_comm().bcast(sums, root=0)

    # ---- whole estimators (bluest_amd.estimator.SamplingMixin) ----------------------------------------------------------------------
    def _field_segments_flushed(self, where, n, segments):
        """rank 0, once per output and flush of _sample_estimators, before the segments are summed: where[i] = (repeat, number of
        the group in the group list) of segments[i] [N, L, d_n] of output n, all ranks' shares joined.  A flush never splits a
        segment.  Nothing is done with them here; bluest_amd.field_errors.FieldErrorsMixin takes their weighted moments."""

    def _sampled_moments_refused(self):
        """no declared weights on the GPU path, so no moments of the drawn samples (FieldErrorsMixin, FieldCovariancesMixin; called
        on the class, whatever the bases are): without SamplingMixin the parent's host flow draws the samples, and an inner product
        written in Python is not a weight vector"""
        return (not isinstance(self, SamplingMixin) or not isinstance(self, FieldOutputsMixin)
                or type(self).get_models_inner_products is not FieldOutputsMixin.get_models_inner_products)

    def _field_group_values(self, col, widths):
        """the step of _sample_estimators that obtains one sampled group col = (g, models, first column, m_g) of one repeat: (per
        output this rank's share of the m_g samples [share, L, d_n], True).  bluest_amd.field_stream.StreamedFieldsMixin returns a
        large group's sums as one row [1, L, d_n] and False: not held, so no flush hook sees it"""
        return draw_field_values(self, col[1], col[3], widths, device_ok=True), True

    def _sample_estimators(self, n_rep):
        """per output mus [n_rep, d_n] of n_rep independent estimators of the current allocation, drawn and flushed as
        SamplingMixin._sample_estimators does, with one field_group_sums call per output and flush"""
        comm = self.get_comm()
        rank = comm.Get_rank()
        cols = sampled_columns(self.MOSAP_output)
        for _, ls, _, _ in cols:
            self._check_field_width(len(ls))
        ws, _ = self._field_weights()
        widths = [len(w) for w in ws]
        W = self._blue_weights()[0] if rank == 0 else None
        mus = [np.zeros((n_rep, d)) for d in widths]

        def draw(col):
            values, held = self._field_group_values(col, widths)
            if comm.Get_size() > 1:
                values = [v.cpu().numpy() if hasattr(v, "data_ptr") else v for v in values]
            return (values, held), col[3] * len(col[1]) * sum(widths) * 8

        def flush(pending, shares):                                     # shares[rank][segment] = (the values per output, held?)
            first, last = pending[0][0], pending[-1][0]
            # every segment brings the weights of its own group
            columns = np.concatenate([np.arange(c, c + len(ls)) for _, (_, ls, c, _) in pending])
            held = [i for i, (_, kept) in enumerate(shares[0]) if kept]
            where = [(pending[i][0], pending[i][1][0]) for i in held]
            for n in range(self.n_outputs):
                joined = [_joined([share[i][0][n] for share in shares]) for i in range(len(pending))]
                if held:                                                # the hooks see the held segments only
                    self._field_segments_flushed(where, n, [joined[i] for i in held])
                _, part = field_group_sums(joined, weights=W[n, columns], repeat_of=[r - first for r, _ in pending], R=last - first + 1)
                mus[n][first:last + 1] += part

        flushed_draws(self, n_rep, cols, SLAB_BYTES, draw, flush)
        return comm.bcast(mus if rank == 0 else None, root=0)

    def solve(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, verbose=True, continuous_relaxation=False,
              max_model_samples=None, optimization_solver_params=None):
        """bluest/blue_models.py:540-576: returns (estimates, their standard errors, total cost); estimates[n] is a float or an
        ndarray [d_n]"""
        if not isinstance(self, SamplingMixin):                         # BLUEProblem's flow over this class's _group_sums
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
        _, is_field = self._field_weights()
        mus = [self._plain(m[0], f) for m, f in zip(self._sample_estimators(1), is_field)]
        Vs = self.comm.bcast(self._blue_weights()[1] if self.mpiRank == 0 else None, root=0)
        return mus, np.sqrt(Vs), self.MOSAP_output["cost"]

    def variance_test(self, budget=None, eps=None, K=3, N=50, **kwargs):
        """bluest/blue_models.py:944-978: N estimators of one allocation; returns (err_ex, err), the error the allocation
        promises and sqrt(s2 / N - <s1, s1> / N^2) with the outputs' inner products"""
        if not isinstance(self, SamplingMixin):
            return super().variance_test(budget=budget, eps=eps, K=K, N=N, **kwargs)
        if budget is None and eps is None:
            raise ValueError("Need to specify either budget or RMSE tolerance")
        elif budget is not None and eps is not None:
            eps = None
        if eps is not None and np.isscalar(eps): eps = [eps for n in range(self.n_outputs)]
        if self.verbose: print("Running variance test...", flush=True)
        self.setup_solver(K=K, budget=budget, eps=eps, **kwargs)
        err_ex = np.sqrt(self.MOSAP_output["variances"])
        err = np.zeros_like(err_ex)
        inners = self.get_models_inner_products()
        _, is_field = self._field_weights()
        mus = self._sample_estimators(int(N))
        for n in range(self.n_outputs):
            s1, s2 = 0, 0.0
            for it in range(int(N)):                                    # the reference's order of additions
                m = self._plain(mus[n][it], is_field[n])
                s1 = s1 + m
                s2 += inners[n](m, m)
            err[n] = np.sqrt(s2 / N - inners[n](s1, s1) / N**2)
        if self.verbose: print("Theoretical error: ", err_ex, flush=True)
        if self.verbose: print("Estimated error:   ", err, flush=True)
        return err_ex, err

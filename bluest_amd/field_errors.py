"""
Sampled error bars for outputs that are vectors ("fields"), in the declared norm and per component.

FieldOutputsMixin.solve() returns the field estimate and the error the MODEL covariance promises, sqrt(e0' Phi^-1 e0), in the inner
product <a, b> = sum_c w_c a_c b_c.  The BLUE weights u_g of a sampled group (SamplingMixin._blue_weights()) are one scalar per
(group, model) column, also for a field, and they are known before the first sample is drawn.  With
z_i[c] = sum_j u_{g,j} y_{g,j}^i[c] for sample i of group g the estimator is mu[c] = sum_g sum_{i <= m_g} z_i[c], so

    Var(mu[c]) = sum_g m_g Var_i(z_i[c])                 the map of the standard error of every component
    E |mu - E mu|^2_w = sum_c w_c Var(mu[c])             the error in the norm, to hold against the promised one

and the unbiased sample variance of z over the m_g samples that were drawn gives unbiased estimates of both, whatever the model
covariance was.  Two sums per (group, component) are all it takes.

field_weighted_moments(values, coef)   per segment [N, L, d] (numpy arrays and CUDA float64 tensors, mixed freely, device tensors
                            read where they lie) and one coefficient per column: (N, zsum [d], zsq [d]), the sums over the samples of
                            z and z^2 with z = sum_j coef_j (y_j - the segment's first sample of y_j), in ONE call on the GPU
                            (bluest_field_weighted_moments, csrc/field_moments.hip).  The order of every operation is fixed
                            (include/bluest_hip.h, Part 15): a segment's bits depend on its values, its coefficients and
                            BLUEST_GSUM_CHUNK only.  There is no CPU path.
variance_of(N, zsum, zsq)   the unbiased variance (zsq - zsum^2 / N) / (N - 1) per component, NaN where N < 2.

FieldErrorsMixin   opt-in, listed first:

    class MyProblem(FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem): ...    # PilotMixin / MLMCMixin may follow

    solve(...)                  FieldOutputsMixin.solve with the same sampler and evaluate calls and the same returned bits; on rank
                                0, after the gather FieldOutputsMixin does anyway, the segments of each flush also go through ONE
                                field_weighted_moments call per output, with that output's BLUE weights.  Afterwards
                                self.field_sample_moments[n][g] = (N, var [d_n]) for every sampled group g of
                                MOSAP_output["flattened_groups"]: the unbiased variance of z, NaN where N < 2.
    sampled_errors(source)      [n_outputs]: sqrt(sum_g m_g sum_c w_c var_g[c]); a group drawn once contributes its model share
                                m_g u_g' C_g u_g.  source="model" gives sqrt(Vs) of solve() again.
    sampled_error_fields()      (maps, unsampled): maps[n] = sqrt(sum_g m_g var_g[c]) over the groups with N >= 2, an ndarray [d_n]
                                (a float for a number); unsampled[n] = the model's variance, in the norm, of the groups that were
                                drawn once and are therefore missing from the map (0.0 when there are none).

A number is a field of one component and goes through the same kernel.  Without SamplingMixin or FieldOutputsMixin among the bases,
or with inner products written in Python, solve() is the parent's and the two new methods refuse.  Still refused (BLUESTError):
sample files and reorder_graph_nodes.
"""
import ctypes

import numpy as np

from . import _lib
from .blue_models import BLUEProblem
from .estimator import SLAB_BYTES, collecting_solve, sampled_columns, sampled_errors
from .fields import FieldOutputsMixin, _field_segment_table
from .sap import BLUESTError


def field_weighted_moments(values, coef, slab_bytes=SLAB_BYTES):
    """list over the segments of (N, zsum [d], zsq [d]): zsum[c] = sum_i z_i[c] and zsq[c] = sum_i z_i[c]^2 with
    z_i[c] = sum_j coef[c0(s) + j] (values[s][i, j, c] - values[s][0, j, c]); coef: [sum of L_s], one finite scalar per column.
    `slab_bytes`: host segments go to the GPU in slabs of whole chunks of at most this size; the result does not depend on it."""
    keep, d, counts, sizes, ptrs, stream = _field_segment_table(values, "field_weighted_moments")
    S, T = len(keep), int(sizes.sum())
    coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64))
    if coef.shape != (T,):
        raise ValueError("coef must have one entry per column: shape [%d]" % T)
    if not np.all(np.isfinite(coef)):
        raise ValueError("coef must be finite")
    zsum, zsq = np.empty((S, d)), np.empty((S, d))
    with _lib.staging_budget(slab_bytes):
        _lib.check(_lib.lib().bluest_field_weighted_moments(S, d, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                                            _lib.ptr(coef), _lib.ptr(zsum), _lib.ptr(zsq), stream))
    return [(int(N), zsum[s].copy(), zsq[s].copy()) for s, N in enumerate(counts.tolist())]


def variance_of(N, zsum, zsq):
    """the unbiased variance [d] of z from the sums of z and z^2 over N samples (the shift drops out); NaN where N < 2"""
    if N < 2:
        return np.full(np.shape(zsum), np.nan)
    return (zsq - zsum * zsum / N) / (N - 1)


class FieldErrorsMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message
    field_sample_moments = None
    _collecting_fields = None

    def _field_segments_flushed(self, where, n, segments):
        if self._collecting_fields is not None:                         # (a variance test's repeats are not looked at)
            W = self._blue_weights()[0]
            col0 = {g: (c, len(ls)) for g, ls, c, _ in sampled_columns(self.MOSAP_output)}
            coef = np.concatenate([W[n, col0[g][0]:col0[g][0] + col0[g][1]] for _, g in where])
            for (_, g), (N, zsum, zsq) in zip(where, field_weighted_moments(segments, coef)):
                self._collecting_fields[n][g] = (N, variance_of(N, zsum, zsq))

    def solve(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, verbose=True, continuous_relaxation=False,
              max_model_samples=None, optimization_solver_params=None):
        """FieldOutputsMixin.solve, and self.field_sample_moments[n] = {group: (N, var [d_n])} of the samples it drew"""
        args = dict(K=K, budget=budget, eps=eps, groups=groups, multi_groups=multi_groups, solver=solver, verbose=verbose,
                    continuous_relaxation=continuous_relaxation, max_model_samples=max_model_samples,
                    optimization_solver_params=optimization_solver_params)
        if FieldOutputsMixin._sampled_moments_refused(self):
            return super().solve(**args)
        result, self.field_sample_moments = collecting_solve(self, super().solve, "_collecting_fields",
                                                             [{} for _ in range(self.n_outputs)], args)
        return result

    def _field_sampled(self):
        if FieldOutputsMixin._sampled_moments_refused(self):
            raise BLUESTError("sampled field errors need SamplingMixin and FieldOutputsMixin among the bases and declared "
                              "output_weights(), not inner products written in Python")
        if self.field_sample_moments is None or self.MOSAP_output is None:
            raise BLUESTError("no field sample moments yet: call solve() first")
        return self.field_sample_moments

    def _model_share(self, n, ls, w):
        """u' C u of a group with the model's covariance in output n's inner product"""
        return float(w @ np.asarray(self.get_covariance(n))[np.ix_(ls, ls)] @ w)

    def sampled_errors(self, source="samples"):
        """[n_outputs]: sqrt(sum_g m_g sum_c w_c var_g[c]) over the sampled groups g, var_g the sampled variance of the group's
        weighted combination z (source="samples"; the model's share u' C u where the group was drawn once), or sqrt(Vs) of solve()
        again (source="model")"""
        def share(sampled, n, g, ls, w):
            moments, ws = sampled
            N, v = moments[n][g]
            return float(np.dot(ws[n], v)) if N >= 2 else self._model_share(n, ls, w)
        return sampled_errors(self, source, lambda: (self._field_sampled(), self._field_weights()[0]), share)

    def sampled_error_fields(self):
        """(maps, unsampled): maps[n][c] = sqrt(sum_g m_g var_g[c]) over the groups drawn at least twice, an ndarray [d_n] or the
        float of a number; unsampled[n] = sum_g m_g u_g' C_g u_g over the groups drawn once, the variance in the norm that the map
        does not show"""
        moments = self._field_sampled()
        comm = self.get_comm()
        result = None
        if comm.Get_rank() == 0:
            W = self._blue_weights()[0]
            ws, is_field = self._field_weights()
            maps, unsampled = [np.zeros(len(w)) for w in ws], [0.0] * self.n_outputs
            for g, ls, c, m in sampled_columns(self.MOSAP_output):
                for n in range(self.n_outputs):
                    w = W[n, c:c + len(ls)]
                    if not w.any():
                        continue
                    N, v = moments[n][g]
                    if N >= 2:
                        maps[n] += m * v
                    else:
                        unsampled[n] += m * self._model_share(n, ls, w)
            result = ([self._plain(np.sqrt(a), f) for a, f in zip(maps, is_field)], unsampled)
        return comm.bcast(result, root=0)

"""
Group covariances of outputs that are vectors ("fields"), from the samples of the main run.

FieldOutputsMixin.solve() draws thousands of joint samples per model group and adds up their columns.  In the declared inner
product <a, b> = sum_c w_c a_c b_c the covariance of a group's models is an L x L matrix, also for a field, and the unbiased sample
covariance of the m_g samples that were drawn estimates it whatever the pilot covariance was: what MomentsMixin gives for plain
numbers, for fields.

field_group_moments(values, w)      per segment [N, L, d] (numpy arrays and CUDA float64 tensors, mixed freely, device tensors read
                            where they lie) and d weights: (N, second [L, L], cross [L, L]), full and symmetric, with
                            second[j, k] = sum_i sum_c w_c d_ij[c] d_ik[c], cross[j, k] = sum_c w_c f_j[c] f_k[c], f_j[c] = sum_i d_ij[c]
                            and d = the values minus the segment's first sample, in ONE call on the GPU
                            (bluest_field_group_moments, csrc/field_cov.hip); with_first=True appends f [L, d].  cross is formed
                            on the device: L (L + 1) doubles per segment travel to the host, the L d per-component sums only on
                            request.  The order of every operation is fixed (include/bluest_hip.h, Part 16): a segment's bits
                            depend on its values, on w, on BLUEST_GSUM_CHUNK and on BLUEST_FIELD_TILE only.  There is no CPU path.
field_group_covariances(values, w)  per segment the unbiased covariance (second - cross / N) / (N - 1) [L, L], NaN where N < 2.

FieldCovariancesMixin   opt-in, listed first:

    class MyProblem(FieldCovariancesMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem): ...   # PilotMixin / MLMCMixin may follow

    solve(...)                  FieldOutputsMixin.solve with the same sampler and evaluate calls and the same returned bits; on rank
                                0, after the gather FieldOutputsMixin does anyway, the segments of each flush also go through ONE
                                field_group_moments call per output.  Afterwards
                                self.field_sample_covariances[n][g] = (N, C^ [L, L]) for every sampled group g of
                                MOSAP_output["flattened_groups"], NaN where N < 2.
    sampled_errors(source)      [n_outputs]: sqrt(sum_g m_g u_g' C^_g u_g) with the BLUE weights u_g; a group drawn once contributes
                                its model share.  source="model" gives sqrt(Vs) of solve() again.
    pooled_covariances()        (Cs, dof) with MomentsMixin's definition, entry for entry: per output the M x M covariance in the
                                inner product pooled over the sampled groups, and the degrees of freedom behind every entry; where
                                no group with two samples holds both models the model's entry stays.  Nothing is projected: the
                                result may be passed on as C to a FieldOutputsMixin problem.

With FieldErrorsMixin in the same class, FieldCovariancesMixin MUST STAND IN FRONT OF IT:

    class MyProblem(FieldCovariancesMixin, FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem): ...

Both hook into _field_segments_flushed.  The hook here passes the segments on to the next class; FieldErrorsMixin's does not chain,
so behind it this mix-in would never see a segment.  (sampled_errors() is then this class's; the two agree to rounding.)

A number is a field of one component and goes through the same kernel.  Without SamplingMixin or FieldOutputsMixin among the bases,
or with inner products written in Python, solve() is the parent's and the new methods refuse.  Still refused (BLUESTError):
sample files and reorder_graph_nodes.
"""
import ctypes

import numpy as np

from . import _lib
from .blue_models import BLUEProblem
from .estimator import SLAB_BYTES, collecting_solve, sampled_errors
from .fields import FieldOutputsMixin, _field_segment_table
from .moments import _triangles_by_width, pool_covariances
from .sap import BLUESTError


def field_group_moments(values, w, with_first=False, slab_bytes=SLAB_BYTES):
    """list over the segments of (N, second [L, L], cross [L, L]) and, with_first, first [L, d]: the sums over the samples of
    <d_j, d_k>, the inner products <f_j, f_k> of f = sum_i d_i, and f itself, with d_i = values[s][i] - values[s][0] and
    <a, b> = sum_c w[c] a[c] b[c]; w: [d] finite weights >= 0.
    `slab_bytes`: host segments go to the GPU in slabs of whole chunks of at most this size; the result does not depend on it."""
    keep, d, counts, sizes, ptrs, stream = _field_segment_table(values, "field_group_moments")
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    if w.shape != (d,):
        raise ValueError("w must have one weight per component: shape [%d]" % d)
    if not np.all(np.isfinite(w)) or np.any(w < 0):
        raise ValueError("the weights must be finite and >= 0")
    T = int(sizes.sum())
    tri = (sizes.astype(np.int64) * (sizes.astype(np.int64) + 1)) // 2
    second, cross = np.empty(int(tri.sum())), np.empty(int(tri.sum()))
    first = np.empty((T, d)) if with_first else None
    with _lib.staging_budget(slab_bytes):
        _lib.check(_lib.lib().bluest_field_group_moments(len(keep), d, _lib.ptr(counts), _lib.ptr(sizes), ctypes.cast(ptrs, ctypes.c_void_p),
                                                         _lib.ptr(w), _lib.ptr(second), _lib.ptr(cross), _lib.ptr(first), stream))
    return _unpacked(counts, sizes, second, cross, first)


def _unpacked(counts, sizes, second, cross, first=None):
    """the outputs of Part 16 ([P], [P] and [T, d] over all segments) as a list of (N, second [L, L], cross [L, L][, first [L, d]]),
    the triangles made full width by width as moments._unpacked does"""
    sizes = sizes.astype(np.int64)
    col0 = np.cumsum(sizes) - sizes
    out = [None] * len(sizes)
    counts = counts.tolist()
    for L, which, at in _triangles_by_width(sizes):
        for s, m2, mx in zip(which.tolist(), np.ascontiguousarray(second[at]), np.ascontiguousarray(cross[at])):
            out[s] = (counts[s], m2, mx) + (() if first is None else (first[col0[s]:col0[s] + L].copy(),))
    return out


def covariance_of(N, second, cross):
    """the unbiased covariance [L, L] in the inner product from the sums of N samples (the shift drops out); NaN where N < 2"""
    if N < 2:
        return np.full(np.shape(second), np.nan)
    return (second - cross / N) / (N - 1)


def field_group_covariances(values, w, slab_bytes=SLAB_BYTES):
    """list over the segments of C^ [L, L] = (second - cross / N) / (N - 1), NaN where N < 2"""
    return [covariance_of(N, second, cross) for N, second, cross in field_group_moments(values, w, slab_bytes=slab_bytes)]


class FieldCovariancesMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message
    field_sample_covariances = None
    _collecting_covariances = None

    def _field_segments_flushed(self, where, n, segments):
        if self._collecting_covariances is not None:                    # (a variance test's repeats are not looked at)
            ws, _ = self._field_weights()
            for (_, g), (N, second, cross) in zip(where, field_group_moments(segments, ws[n])):
                self._collecting_covariances[n][g] = (N, covariance_of(N, second, cross))
        super()._field_segments_flushed(where, n, segments)                # FieldErrorsMixin may stand behind: it sees them too

    def solve(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, verbose=True, continuous_relaxation=False,
              max_model_samples=None, optimization_solver_params=None):
        """FieldOutputsMixin.solve, and self.field_sample_covariances[n] = {group: (N, C^ [L, L])} of the samples it drew"""
        args = dict(K=K, budget=budget, eps=eps, groups=groups, multi_groups=multi_groups, solver=solver, verbose=verbose,
                    continuous_relaxation=continuous_relaxation, max_model_samples=max_model_samples,
                    optimization_solver_params=optimization_solver_params)
        if FieldOutputsMixin._sampled_moments_refused(self):
            return super().solve(**args)
        result, self.field_sample_covariances = collecting_solve(self, super().solve, "_collecting_covariances",
                                                                 [{} for _ in range(self.n_outputs)], args)
        return result

    def _field_covariances_sampled(self):
        if FieldOutputsMixin._sampled_moments_refused(self):
            raise BLUESTError("sampled field covariances need SamplingMixin and FieldOutputsMixin among the bases and declared "
                              "output_weights(), not inner products written in Python")
        if self.field_sample_covariances is None or self.MOSAP_output is None:
            raise BLUESTError("no field sample covariances yet: call solve() first")
        return self.field_sample_covariances

    def sampled_errors(self, source="samples"):
        """[n_outputs]: sqrt(sum_g m_g u_g' C_g u_g) over the sampled groups g, u_g the BLUE weights of the group's columns and C_g
        the covariance of the group's samples in the inner product (source="samples"; the model's block where the group was drawn
        once), or sqrt(Vs) of solve() again (source="model")"""
        def share(covs, n, g, ls, u):
            N, C_hat = covs[n][g]
            C = C_hat if N >= 2 else np.asarray(self.get_covariance(n))[np.ix_(ls, ls)]
            return float(u @ C @ u)
        return sampled_errors(self, source, self._field_covariances_sampled, share)

    def pooled_covariances(self):
        """(Cs, dof) with MomentsMixin's definition, entry for entry, in the outputs' inner products"""
        return pool_covariances(self, self._field_covariances_sampled())

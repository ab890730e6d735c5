"""
Second moments of a sampled allocation, and the error bar they imply.

SamplingMixin.solve() draws thousands of joint samples per model group, adds up their columns and reports the standard error the
MODEL covariance promises, sqrt(e0' Phi^-1 e0).  With the weights w[o][g] = C_{o,g}^-1 R_g v_o of SamplingMixin._blue_weights()
the estimator is mu_o = sum_g sum_{i <= m_g} w[o][g]' y_g^i over independent samples, so

    Var(mu_o) = sum_g m_g w[o][g]' Cov(y_g) w[o][g].

With the model blocks C_{o,g} for Cov(y_g) this is e0' Phi^-1 e0 again; with the unbiased sample covariance of the m_g samples
that were drawn it is an unbiased estimate of the estimator's true variance, whatever the model covariance was.

group_moments(values)       per segment [n_out, N, L] (numpy arrays and CUDA float64 tensors, mixed freely, device tensors read where
                            they lie): (N, first [n_out, L], second [n_out, L, L]), the sums of d and of d d' with d = the values
                            minus the segment's first sample, in ONE call on the GPU (bluest_group_moments, csrc/moments.hip).  The
                            order of every operation is fixed (include/bluest_hip.h, Part 13): a segment's bits depend on its values
                            and on BLUEST_GSUM_CHUNK only.
group_covariances(values)   per segment the unbiased sample covariance [n_out, L, L] (NaN where N < 2).

MomentsMixin   opt-in, listed first:

    class MyProblem(MomentsMixin, SamplingMixin, BLUEProblem): ...       # PilotMixin / MLMCMixin may follow SamplingMixin

    solve(...)                  SamplingMixin.solve with the same sampler calls and the same returned bits; the segments of the draw
                                also go through group_moments (on rank 0, after the gather SamplingMixin does anyway).  Afterwards
                                self.sample_moments[g] = (N, C^ [n_outputs, L, L]) for every sampled group g of
                                MOSAP_output["flattened_groups"].
    sampled_errors(source)      [n_outputs]: sqrt(sum_g m_g w' C^ w); a group drawn once contributes its model block.
                                source="model" takes the model blocks throughout and gives sqrt(Vs) of solve() again.
    pooled_covariances()        (Cs, dof): per output the M x M covariance pooled over the sampled groups, and the degrees of freedom
                                behind every entry; where no group with two samples holds both models the model's entry stays.
                                Nothing is projected: the result may be passed on as C.

Outputs that are not plain numbers (inner products written in Python, or FieldOutputsMixin among the bases) keep their parent's
solve(), and the two new methods refuse.  Still refused (BLUESTError): sample files and reorder_graph_nodes.
"""
import ctypes
import functools

import numpy as np

from . import _lib
from .blue_models import BLUEProblem
from .estimator import SLAB_BYTES, _segment_table, collecting_solve, sampled_errors
from .sap import BLUESTError


def group_moments(values, slab_bytes=SLAB_BYTES):
    """list over the segments of (N, first [n_out, L], second [n_out, L, L]): first[n, j] = sum_i d[n, i, j] and
    second[n, j, k] = sum_i d[n, i, j] d[n, i, k] (full, symmetric) with d[n, i, :] = values[n, i, :] - values[n, 0, :].
    `slab_bytes`: host segments go to the GPU in slabs of whole chunks of at most this size; the result does not depend on it."""
    keep, n_out, counts, sizes, ptrs, stream = _segment_table(values, "group_moments")
    T = int(sizes.sum())
    tri = (sizes.astype(np.int64) * (sizes.astype(np.int64) + 1)) // 2
    first, second = np.empty((n_out, T)), np.empty((n_out, int(tri.sum())))
    with _lib.staging_budget(slab_bytes):
        _lib.check(_lib.lib().bluest_group_moments(len(keep), n_out, _lib.ptr(counts), _lib.ptr(sizes),
                                                   ctypes.cast(ptrs, ctypes.c_void_p), _lib.ptr(first), _lib.ptr(second), stream))
    return _unpacked(counts, sizes, first, second)


@functools.lru_cache(maxsize=None)
def _triangle(L):
    """[L, L]: where the pair (j, k) lies in the packed order of Part 13 (row-major over j <= k), for either order of j and k"""
    j, k = np.triu_indices(L)
    at = np.empty((L, L), dtype=np.int64)
    at[j, k] = at[k, j] = np.arange(len(j))
    return at


def _triangles_by_width(sizes):
    """per width L among the segments' `sizes`: (L, the segments of that width, where their pairs lie in the packed triangles of
    all segments, [segment, L, L]).  Indexing with it turns packed triangles into full symmetric matrices width by width, not
    segment by segment: a variance test's batch has thousands."""
    sizes = sizes.astype(np.int64)
    tri = sizes * (sizes + 1) // 2
    pair0 = np.cumsum(tri) - tri
    for L in set(sizes.tolist()):
        which = np.flatnonzero(sizes == L)
        yield L, which, pair0[which][:, None, None] + _triangle(L)


def _unpacked(counts, sizes, first, second):
    """the outputs of Part 13 ([n_out, T] and [n_out, P] over all segments) as a list of (N, first [n_out, L], second [n_out, L, L])"""
    sizes = sizes.astype(np.int64)
    col0 = np.cumsum(sizes) - sizes
    out = [None] * len(sizes)
    counts = counts.tolist()
    for L, which, at in _triangles_by_width(sizes):
        square = second[:, at].transpose(1, 0, 2, 3)                                            # [segment, n_out, L, L]
        cols = first[:, col0[which][:, None] + np.arange(L)].transpose(1, 0, 2)                 # [segment, n_out, L]
        for s, f, m in zip(which.tolist(), np.ascontiguousarray(cols), np.ascontiguousarray(square)):
            out[s] = (counts[s], f, m)
    return out


def covariance_of(N, first, second):
    """the unbiased sample covariance [n_out, L, L] from the sums of d and d d' of N samples (the shift drops out); NaN where N < 2"""
    if N < 2:
        return np.full(second.shape, np.nan)
    return (second - first[:, :, None] * first[:, None, :] / N) / (N - 1)


def group_covariances(values, slab_bytes=SLAB_BYTES):
    """list over the segments of C^ [n_out, L, L] = (second - first first' / N) / (N - 1), NaN where N < 2"""
    return [covariance_of(N, first, second) for N, first, second in group_moments(values, slab_bytes=slab_bytes)]


def pool_covariances(problem, sampled):
    """(Cs, dof) of pooled_covariances() from sampled[n] = {group: (N, C^ [L, L])} of output n"""
    groups = problem.MOSAP_output["flattened_groups"]
    Cs, dofs = [], []
    for n in range(problem.n_outputs):
        acc, dof = np.zeros((problem.M, problem.M)), np.zeros((problem.M, problem.M))
        for g, (N, C_hat) in sorted(sampled[n].items()):
            if N >= 2:
                ix = np.ix_(groups[g], groups[g])
                acc[ix] += (N - 1) * C_hat
                dof[ix] += N - 1
        C = np.array(problem.get_covariance(n), dtype=np.float64)
        C[dof > 0] = acc[dof > 0] / dof[dof > 0]
        Cs.append(C)
        dofs.append(dof)
    return Cs, dofs


class MomentsMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message
    sample_moments = None
    _collecting = None

    def _moments_refused(self):
        """outputs that are not plain numbers: no second moments on the GPU"""
        from .fields import FieldOutputsMixin
        return isinstance(self, FieldOutputsMixin) or self._host_outputs()

    def _segments_flushed(self, where, segments):
        if self._collecting is not None:                                # (a variance test's repeats are not looked at)
            for (_, g), v, C in zip(where, segments, group_covariances(segments)):
                self._collecting[g] = (int(v.shape[1]), C)

    def solve(self, K=4, budget=None, eps=None, groups=None, multi_groups=None, solver=None, verbose=True, continuous_relaxation=False,
              max_model_samples=None, optimization_solver_params=None):
        """SamplingMixin.solve, and self.sample_moments = {group: (N, C^ [n_outputs, L, L])} of the samples it drew"""
        args = dict(K=K, budget=budget, eps=eps, groups=groups, multi_groups=multi_groups, solver=solver, verbose=verbose,
                    continuous_relaxation=continuous_relaxation, max_model_samples=max_model_samples,
                    optimization_solver_params=optimization_solver_params)
        if self._moments_refused():
            return super().solve(**args)
        result, self.sample_moments = collecting_solve(self, super().solve, "_collecting", {}, args)
        return result

    def _sampled(self):
        if self._moments_refused():
            raise BLUESTError("sample moments cover outputs that are plain numbers: not inner products written in Python, not fields")
        if self.sample_moments is None or self.MOSAP_output is None:
            raise BLUESTError("no sample moments yet: call solve() first")
        return self.sample_moments

    def sampled_errors(self, source="samples"):
        """[n_outputs]: sqrt(sum_g m_g w' C w) over the sampled groups g, w the BLUE weights of the group's columns and C the
        covariance of the group's samples (source="samples"; the model's block where the group was drawn once) or the model's
        block throughout (source="model": sqrt(Vs) of solve() again)"""
        def share(moments, n, g, ls, w):
            N, C_hat = moments[g]
            C = C_hat[n] if source == "samples" and N >= 2 else self.get_covariance(n)[np.ix_(ls, ls)]
            return w @ C @ w
        return sampled_errors(self, source, self._sampled, share, promised=False)

    def pooled_covariances(self):
        """(Cs, dof), per output M x M: dof[i, j] = sum of N_g - 1 over the sampled groups with N_g >= 2 that hold both i and j,
        Cs[i, j] = sum (N_g - 1) C^_g[i, j] / dof[i, j] where dof > 0, elsewhere the entry of get_covariance(n) (NaN included)"""
        moments = self._sampled()
        return pool_covariances(self, [{g: (N, C_hat[n]) for g, (N, C_hat) in moments.items()} for n in range(self.n_outputs)])

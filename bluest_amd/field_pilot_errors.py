"""
Standard errors of the pilot estimates of field outputs, and a field pilot that grows until they are small enough: what
bluest_amd.pilot_errors does for numbers, for outputs that are vectors with a declared inner product (bluest_amd.fields).

A pilot sample of a field costs L PDE solves, so params["covariance_estimation_samples"] is an expensive guess.  The covariance
estimate is the mean over the samples of the per-sample inner product of the centred fields,

    C^_ij = mean_s q_s(i, j),   q_s(i, j) = <y_i^s - a_i, y_j^s - a_j>_w,   a = the per-component mean,

and likewise dV^_ij = mean_s r_s(i, j) with r_s the squared norm of the centred explicit difference.  Their standard errors are
the standard errors of these means: with u_s = q_s - q_0, S1 = sum u_s, S2 = sum u_s^2,

    SE(C^_ij) = sqrt(max(S2 - S1^2 / N, 0) / (N (N - 1))),          the same from r_s for SE(dV^_ij);  N < 2: NaN.

This is the FIRST-ORDER (delta-method) error: the centre is treated as known.  The O(1 / N) relative terms that the scalar formula
of pilot_standard_errors keeps would need the d x d covariances of the components, which nobody forms; at d = 1 the two differ by
about 1 / N relatively.

field_pilot_moments(values, w, centre=None, differences=True)
    values [N, L, d] (numpy or a CUDA float64 tensor, read in place), w [d] >= 0, centre [L, d] (default: the mean, from
    field_statistics) -> (qfirst, qs1, qs2, rfirst, rs1, rs2), each [L, L]: q_0, sum (q_s - q_0), sum (q_s - q_0)^2, symmetric, and
    the same of r at i < j (0 elsewhere; None without differences), on the GPU (bluest_field_pilot_moments, csrc/field_pilot.hip).
    The order of every operation is fixed (include/bluest_hip.h, Part 17): the same bits from host or device memory, under any
    staging budget and scratch limit.  There is no CPU path.
field_pilot_standard_errors(N, qs1, qs2, rs1=None, rs2=None)
    (SE(C^) [L, L], SE(dV^) [L, L] at i < j, NaN elsewhere; None without rs1 / rs2)

FieldPilotErrorsMixin   opt-in, listed first:

    class MyProblem(FieldPilotErrorsMixin, FieldOutputsMixin, PilotMixin, BLUEProblem): ...

    MyProblem(M, ..., covariance_estimation_samples=100)        # FieldOutputsMixin's sampler calls and the bits of C and dV; one
                                                                # field_pilot_moments call per output on the same values follows
    MyProblem(M, ..., covariance_estimation_tol=0.1)            # the pilot grows (pilot_errors.next_pilot_size) until every
                                                                # estimated coupled entry has SE(C^_ij) <= tol sqrt(C^_ii C^_jj) and
                                                                # SE(dV^_ij) <= tol dV^_ij, or covariance_estimation_max_samples
                                                                # (default 64 x the initial size) or covariance_estimation_max_bytes
                                                                # (default 2 GiB for the kept values of the largest output) is reached

    get_covariance_errors(), get_covariance_error(n), get_mlmc_variance_errors(), get_mlmc_variance_error(n)
    pilot_report = {"samples", "rounds", "ratio", "converged", "capped_by": None | "samples" | "bytes"}

Every round draws only what is missing.  Rank 0 keeps the values drawn so far, round-major and then in rank order, in the memory
they arrived in (CUDA tensors stay on the device; a change of residence between rounds raises BLUESTError), and computes C and dV
from one field_statistics call over all of them: the final result is bit for bit what FieldOutputsMixin gives on those values.  A
number among the outputs (output_weights() entry None) is a field of one component.  Inner products written in Python and
problems loaded from a model-graph file are refused as PilotErrorsMixin refuses them: with a tolerance the constructor raises,
without one the mix-in behaves as its bases and the accessors refuse.
"""
import contextlib
import ctypes

import numpy as np

from . import _lib
from .estimator import SLAB_BYTES
from .fields import FieldOutputsMixin, _segment, _stream_of, field_statistics
from .pilot_errors import _GrowingPilot
from .sap import BLUESTError

BLUEST_FIELD_STRIP = 512             # include/bluest_hip.h, Part 17
MAX_BYTES = 2 << 30                  # default of covariance_estimation_max_bytes


@contextlib.contextmanager
def scratch_limit(scratch_bytes):
    """with scratch_limit(scratch_bytes): ... -- field_pilot_moments calls inside keep their per-sample device scratch under
    `scratch_bytes` (bluest_field_pilot_scratch; None leaves the limit alone).  The limit is process-wide: it is left as it was."""
    if scratch_bytes is None:
        yield
        return
    before = _lib.c_i64(0)
    _lib.check(_lib.lib().bluest_field_pilot_scratch(max(int(scratch_bytes), 1), ctypes.byref(before)))
    try:
        yield
    finally:
        _lib.lib().bluest_field_pilot_scratch(before.value, None)


def field_pilot_moments(values, w, centre=None, differences=True, slab_bytes=SLAB_BYTES, scratch_bytes=None):
    """(qfirst, qs1, qs2, rfirst, rs1, rs2) [L, L] as numpy arrays from values[s, i, c] = component c of model i on sample s, the
    weights w [d] and the centre [L, d] (default: field_statistics(values, w, differences=False)[0] / N); the r arrays are None
    when `differences` is False.  The result depends on neither `slab_bytes` nor `scratch_bytes`."""
    values = _segment(values, "values")
    N, L, d = (int(x) for x in values.shape)
    w = np.ascontiguousarray(np.asarray(w, dtype=np.float64))
    if w.shape != (d,):
        raise ValueError("w must have one weight per component: shape [%d]" % d)
    if centre is None:
        centre = field_statistics(values, w, differences=False)[0] / N
    centre = np.ascontiguousarray(np.asarray(centre, dtype=np.float64))
    if centre.shape != (L, d):
        raise ValueError("centre must have the shape [%d, %d]" % (L, d))
    out = [np.empty((L, L)) for _ in range(6 if differences else 3)] + [None] * (0 if differences else 3)
    stream = _stream_of(values) if hasattr(values, "data_ptr") else None
    with _lib.staging_budget(slab_bytes), scratch_limit(scratch_bytes):
        _lib.check(_lib.lib().bluest_field_pilot_moments(N, L, d, _lib.ptr(values), _lib.ptr(w), _lib.ptr(centre),
                                                         *([_lib.ptr(a) for a in out] + [stream])))
    return tuple(out)


def _sem(N, s1, s2):
    s1, s2 = np.asarray(s1, dtype=np.float64), np.asarray(s2, dtype=np.float64)
    return np.sqrt(np.maximum(s2 - s1 * s1 / N, 0.0) / (N * (N - 1)))


def field_pilot_standard_errors(N, qs1, qs2, rs1=None, rs2=None):
    """(SE(C^) [L, L], SE(dV^) [L, L] or None without rs1 / rs2) from the sums of field_pilot_moments over N samples: the standard
    error of the mean of q_s and of r_s, sqrt(max(S2 - S1^2 / N, 0) / (N (N - 1))).  SE(dV^) is NaN outside i < j; N < 2 gives
    NaN everywhere.  First order: see the module's docstring."""
    N = int(N)
    shape = np.shape(qs1)
    with_r = rs1 is not None and rs2 is not None
    if N < 2:
        return np.full(shape, np.nan), (np.full(shape, np.nan) if with_r else None)
    se_c = _sem(N, qs1, qs2)
    if not with_r:
        return se_c, None
    se_d = _sem(N, rs1, rs2)
    se_d[~np.triu(np.ones(shape, dtype=bool), 1)] = np.nan
    return se_c, se_d


class FieldPilotErrorsMixin(_GrowingPilot):
    _pilot_needs = "the per-sample inner products of declared weights"
    _pilot_sumse = None                  # the sums of the components the last _pilot_sums returned

    def _pilot_unavailable(self):
        """why the per-sample inner products do not come from bluest_field_pilot_moments, or None"""
        if not isinstance(self, FieldOutputsMixin):
            return "FieldOutputsMixin is not among the bases"
        if type(self).get_models_inner_products is not FieldOutputsMixin.get_models_inner_products:
            return "inner products written in Python are summed on the host"
        return None

    def _pilot_caps(self, ls, N, size):
        ws, _ = self._field_weights()
        by_samples = max(N, int(self.params.get("covariance_estimation_max_samples", 64 * N)))
        per_sample = len(ls) * max(len(w) for w in ws) * 8              # the kept values of the largest output
        by_bytes = max(N, int(self.params.get("covariance_estimation_max_bytes", MAX_BYTES)) // per_sample // size * size)
        return min(by_samples, by_bytes), "bytes" if by_bytes < by_samples else "samples"

    def _pilot_reset(self):
        super()._pilot_reset()
        self._pilot_sumse = None

    def _pilot_reported(self, samples, rounds, ratio, converged, cap):
        return dict(super()._pilot_reported(samples, rounds, ratio, converged, cap), capped_by=cap)

    # ---- FieldOutputsMixin's hooks: a round draws what is missing, rank 0 keeps what was drawn, per output [N, L, d_n] ----------------
    def _field_pilot_count(self, ls, N):
        return N - self._pilot_have

    def _field_pilot_gathered(self, ls, values):
        if self._pilot_kept is not None:
            joined = []
            for n, (old, new) in enumerate(zip(self._pilot_kept, values)):
                if hasattr(old, "data_ptr") != hasattr(new, "data_ptr"):
                    raise BLUESTError("output %d arrived in %s memory in this round of the pilot and in %s memory before"
                                      % (n, *("device" if hasattr(v, "data_ptr") else "host" for v in (new, old))))
                if hasattr(old, "data_ptr"):
                    import torch
                    joined.append(torch.cat([old, new], dim=0))         # round-major, then in rank order
                else:
                    joined.append(np.concatenate([old, new], axis=0))
            values = joined
        self._pilot_kept = values
        return values

    def _pilot_sums(self, ls, N):
        sums = super()._pilot_sums(ls, N)
        self._pilot_sumse = sums[0]
        return sums

    def _pilot_round(self, ls, N, estimates):
        """one field_pilot_moments call per output, centred at the mean field_statistics returned; C^ and dV^ are the means of the
        per-sample inner products q_s and r_s"""
        L = len(ls)
        ws, _ = self._field_weights()
        se_c, se_d = np.empty((self.n_outputs, L, L)), np.empty((self.n_outputs, L, L))
        C_hat, dV_hat = (np.empty((self.n_outputs, L, L)), np.empty((self.n_outputs, L, L))) if estimates else (None, None)
        for n in range(self.n_outputs):
            centre = np.array([np.atleast_1d(np.asarray(self._pilot_sumse[n][i], dtype=np.float64)) for i in range(L)]) / N
            qfirst, qs1, qs2, rfirst, rs1, rs2 = field_pilot_moments(self._pilot_kept[n], ws[n], centre, differences=True)
            se_c[n], se_d[n] = field_pilot_standard_errors(N, qs1, qs2, rs1, rs2)
            if estimates:
                C_hat[n], dV_hat[n] = qfirst + qs1 / N, rfirst + rs1 / N
        return se_c, se_d, C_hat, dV_hat

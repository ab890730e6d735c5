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
from .blue_models import BLUEProblem
from .estimator import SLAB_BYTES
from .fields import FieldOutputsMixin, _segment, _stream_of, field_statistics
from .pilot_errors import PilotErrorsMixin, next_pilot_size
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


class FieldPilotErrorsMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message
    pilot_report = None
    _pilot_errors = None                 # (errors of C [n_outputs, M, M], errors of dV [n_outputs, M, M])
    _pilot_kept = None                   # rank 0, while the pilot runs: per output the values drawn so far [N, L, d_n]
    _pilot_have = 0                      # every rank: how many samples the values kept on rank 0 hold
    _pilot_sumse = None                  # the sums of the components the last _pilot_sums returned

    _pilot_tol = PilotErrorsMixin._pilot_tol

    def _no_field_moments(self):
        """why the per-sample inner products do not come from bluest_field_pilot_moments, or None"""
        if not isinstance(self, FieldOutputsMixin):
            return "FieldOutputsMixin is not among the bases"
        if type(self).get_models_inner_products is not FieldOutputsMixin.get_models_inner_products:
            return "inner products written in Python are summed on the host"
        return None

    # ---- BLUEProblem's hooks ----------------------------------------------------------------------------------------------------
    def _init_inputs(self, C, costs):
        why = self._no_field_moments()
        if why is not None and self._pilot_tol() is not None:
            raise BLUESTError("covariance_estimation_tol needs the per-sample inner products of declared weights: " + why)
        return super()._init_inputs(C, costs)

    def _init_from_datafile(self, datafile, costs):
        if self._pilot_tol() is not None:
            raise BLUESTError("covariance_estimation_tol needs pilot samples: a problem loaded from a model-graph file draws none")
        return super()._init_from_datafile(datafile, costs)

    # ---- FieldOutputsMixin's hooks: a round draws what is missing, rank 0 keeps what was drawn ---------------------------------------
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

    def estimate_missing_covariances(self, N):
        """FieldOutputsMixin's estimate_missing_covariances, then the standard errors of what it estimated; with
        params["covariance_estimation_tol"] the pilot grows from N samples until the errors meet the tolerance"""
        if self._no_field_moments() is not None:
            return super().estimate_missing_covariances(N)
        unknown = [cp.linked & np.isnan(cp.cov) for cp in self._coupling]
        ls = [int(l) for l in np.flatnonzero(np.logical_or.reduce(unknown).any(axis=1))]
        no_dV = [~np.isfinite(np.array(d, dtype=np.float64)) for d in self.dV]
        nan = lambda: np.full((self.n_outputs, self.M, self.M), np.nan)
        if len(ls) == 0:                                                # nothing to estimate: nothing has an error
            if self._pilot_errors is None:
                self._pilot_errors = (nan(), nan())
                self.pilot_report = dict(samples=0, rounds=0, ratio=None, converged=True, capped_by=None)
            return
        self._pilot_errors = (nan(), nan())
        tol, comm = self._pilot_tol(), self.get_comm()
        size, N = comm.Get_size(), int(N)
        ws, _ = self._field_weights()
        by_samples = max(N, int(self.params.get("covariance_estimation_max_samples", 64 * N)))
        per_sample = len(ls) * max(len(w) for w in ws) * 8              # the kept values of the largest output
        by_bytes = max(N, int(self.params.get("covariance_estimation_max_bytes", MAX_BYTES)) // per_sample // size * size)
        N_max = min(by_samples, by_bytes)
        before = ([cp.cov.copy() for cp in self._coupling], [np.array(d, dtype=np.float64) for d in self.dV])
        rounds = 0
        try:
            while True:
                for cp, cov in zip(self._coupling, before[0]):         # every round estimates from the inputs as they were given
                    cp.cov[...] = cov
                self.dV = [d.copy() for d in before[1]]
                super().estimate_missing_covariances(N)
                rounds += 1
                self._pilot_have = N
                found = None
                if comm.Get_rank() == 0:
                    found = self._pilot_round(ls, N, ws, unknown, no_dV, tol)
                se_c, se_d, ratio = comm.bcast(found, root=0)
                more = None
                if comm.Get_rank() == 0:                                # rank 0 decides
                    more = next_pilot_size(N, ratio, size, N_max) if tol is not None and ratio > 1 and N < N_max else N
                more = comm.bcast(more, root=0)
                if more == N:
                    break
                N = more
        finally:
            self._pilot_kept, self._pilot_have, self._pilot_sumse = None, 0, None
        where = np.ix_(range(self.n_outputs), ls, ls)
        self._pilot_errors[0][where] = se_c
        self._pilot_errors[1][where] = se_d
        for n in range(self.n_outputs):
            self._pilot_errors[0][n][~unknown[n]] = np.nan              # given, not estimated
            self._pilot_errors[1][n][~(no_dV[n] & np.triu(np.ones((self.M, self.M), dtype=bool), 1))] = np.nan
        converged = tol is None or ratio <= 1
        capped_by = None if converged else ("bytes" if by_bytes < by_samples else "samples")
        self.pilot_report = dict(samples=N, rounds=rounds, ratio=float(ratio) if tol is not None else None, converged=converged,
                                 capped_by=capped_by)
        if not converged and comm.Get_rank() == 0:
            print("WARNING! The pilot estimates miss covariance_estimation_tol = %g after %d samples (largest error / tolerance: "
                  "%.3g). Raise covariance_estimation_max_%s." % (tol, N, ratio, capped_by))

    def _pilot_round(self, ls, N, ws, unknown, no_dV, tol):
        """rank 0: (SE(C^), SE(dV^)) [n_outputs, L, L] of the values kept, from one field_pilot_moments call per output centred at
        the mean field_statistics returned, and the largest ratio of an error to what the tolerance allows over the estimated
        coupled entries (0 without a tolerance)"""
        L = len(ls)
        se_c, se_d = np.empty((self.n_outputs, L, L)), np.empty((self.n_outputs, L, L))
        ratio = 0.0
        sub = np.ix_(ls, ls)
        for n in range(self.n_outputs):
            centre = np.array([np.atleast_1d(np.asarray(self._pilot_sumse[n][i], dtype=np.float64)) for i in range(L)]) / N
            qfirst, qs1, qs2, rfirst, rs1, rs2 = field_pilot_moments(self._pilot_kept[n], ws[n], centre, differences=True)
            se_c[n], se_d[n] = field_pilot_standard_errors(N, qs1, qs2, rs1, rs2)
            if tol is None:
                continue
            C_hat, dV_hat = qfirst + qs1 / N, rfirst + rs1 / N         # the means of q_s and r_s
            var = np.diagonal(C_hat)
            scale = np.sqrt(np.outer(var, var))
            use = unknown[n][sub] & (scale > 0)
            pairs = (no_dV[n] & self._coupling[n].linked)[sub] & np.triu(np.ones(scale.shape, dtype=bool), 1) & (dV_hat > 0) & (scale > 0)
            for err, ref, mask in ((se_c[n], scale, use), (se_d[n], dV_hat, pairs)):
                if mask.any():
                    r = err[mask] / (tol * ref[mask])
                    ratio = max(ratio, float(np.inf if np.isnan(r).any() else r.max()))
        return se_c, se_d, ratio

    # ---- what was measured --------------------------------------------------------------------------------------------------------
    def _errors(self):
        if self._pilot_errors is None:
            why = self._no_field_moments() or "nothing was estimated from pilot samples (a problem loaded from a model-graph file?)"
            raise BLUESTError("no standard errors of the pilot estimates: " + why)
        return self._pilot_errors

    get_covariance_errors = PilotErrorsMixin.get_covariance_errors
    get_covariance_error = PilotErrorsMixin.get_covariance_error
    get_mlmc_variance_errors = PilotErrorsMixin.get_mlmc_variance_errors
    get_mlmc_variance_error = PilotErrorsMixin.get_mlmc_variance_error

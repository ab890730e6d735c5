"""
Standard errors of the pilot estimates, and a pilot that grows until they are small enough.

Everything BLUEProblem computes rests on the covariances C and the MLMC difference variances dV that PilotMixin estimates from
params["covariance_estimation_samples"] pilot samples (default 100): a guess that nothing checked.  The sampling error of every
estimated entry follows from the fourth moments of the same samples, one more pass over the array that is already on the device.

pilot_fourth_moments(values)    (shift, first, s11, s21, s22, tpow): with d = values - shift, the sums over the samples of d_i,
                                d_i d_j, d_i^2 d_j, d_i^2 d_j^2 and -- from the explicit differences, t = (y_i - y_j) - (a_i - a_j) --
                                of t, t^2, t^3, t^4, on the GPU (bluest_pilot_moments4, csrc/pilot4.hip).  The order of every
                                operation is fixed (include/bluest_hip.h, Part 14): the bits depend on the values, the shift and
                                BLUEST_PILOT_CHUNK only.
pilot_standard_errors(N, ...)   (SE(C^) [n_out, L, L], SE(dV^) [n_out, L, L] at i < j) of the 1/N estimates PilotMixin writes.

PilotErrorsMixin   opt-in, listed first:

    class MyProblem(PilotErrorsMixin, PilotMixin, BLUEProblem): ...

    MyProblem(M, ..., covariance_estimation_samples=100)                  # PilotMixin's sampler calls, C and dV bits; one
                                                                          # pilot_fourth_moments call on the same values follows
    MyProblem(M, ..., covariance_estimation_tol=0.1)                      # the pilot grows until every estimated coupled entry has
                                                                          # SE(C^_ij) <= tol sqrt(C^_ii C^_jj) and SE(dV^_ij) <= tol dV^_ij,
                                                                          # or covariance_estimation_max_samples (default 64 x the
                                                                          # initial size) is reached

    get_covariance_errors(), get_covariance_error(n), get_mlmc_variance_errors(), get_mlmc_variance_error(n)
    pilot_report = {"samples", "rounds", "ratio", "converged"}

Outputs that are not plain numbers (inner products written in Python, FieldOutputsMixin among the bases) and problems loaded
from a model-graph file have no sums from bluest_pilot_stats: with a tolerance the constructor refuses, without one the mix-in
behaves as PilotMixin and the accessors refuse.  Still refused (BLUESTError): sample files and reorder_graph_nodes.
"""
import ctypes
import math

import numpy as np

from . import _lib
from .blue_models import BLUEProblem
from .pilot import BLUEST_PILOT_CHUNK, SLAB_BYTES, next_divisible_number
from .sap import BLUESTError


def _moments4_call(values, N, L, n_out, shift, differences, stream):
    first = np.empty((n_out, L))
    s11, s21, s22 = np.empty((n_out, L, L)), np.empty((n_out, L, L)), np.empty((n_out, L, L))
    tpow = np.empty((n_out, 4, L, L)) if differences else None
    _lib.check(_lib.lib().bluest_pilot_moments4(N, L, n_out, _lib.ptr(values), _lib.ptr(shift), _lib.ptr(first), _lib.ptr(s11),
                                                _lib.ptr(s21), _lib.ptr(s22), _lib.ptr(tpow), stream))
    return first, s11, s21, s22, tpow


def _checked_shift(shift, n_out, L):
    if shift is None:
        return None
    shift = np.ascontiguousarray(shift, dtype=np.float64)
    if shift.shape != (n_out, L):
        raise ValueError("shift must have the shape [n_outputs, L]")
    return shift


def pilot_fourth_moments(values, differences=True, shift=None, slab_bytes=SLAB_BYTES):
    """(shift_used [n_out, L], first [n_out, L], s11, s21, s22 [n_out, L, L], tpow [n_out, 4, L, L]) as numpy arrays from
    values[n, s, i] = output n of model i on sample s: a numpy array or a CUDA torch tensor of shape [n_out, N, L] (float64); a
    device tensor is read in place on the current stream.  With d = values - shift (default: the first sample): first = sum d_i,
    s11 = sum d_i d_j, s21[i, j] = sum d_i^2 d_j, s22 = sum d_i^2 d_j^2; tpow[:, k - 1] holds sum t^k at i < j and 0 elsewhere,
    t = (y_i - y_j) - (shift_i - shift_j) from the explicit differences, and is None when `differences` is False.  A host array of
    more than `slab_bytes` is fed output by output in slabs of whole chunks of BLUEST_PILOT_CHUNK samples, all with the shift of
    the first slab, and the slabs' sums are added in order: a function of the values, BLUEST_PILOT_CHUNK and `slab_bytes` only."""
    if hasattr(values, "data_ptr"):                                     # a torch tensor
        import torch
        if values.dim() != 3 or values.dtype != torch.float64:
            raise ValueError("values must be a float64 array of shape [n_outputs, N, L]")
        if not values.is_cuda:
            values = values.numpy()
        else:
            values = values.contiguous()
            n_out, N, L = (int(d) for d in values.shape)
            shift = _checked_shift(shift, n_out, L)
            with torch.cuda.device(values.device):
                stream = ctypes.c_void_p(torch.cuda.current_stream().cuda_stream)
                used = values[:, 0, :].cpu().numpy() if shift is None and N > 0 else shift
                return (used,) + _moments4_call(values, N, L, n_out, shift, differences, stream)
    values = np.asarray(values, dtype=np.float64)
    if values.ndim != 3:
        raise ValueError("values must be a float64 array of shape [n_outputs, N, L]")
    n_out, N, L = values.shape
    values = np.ascontiguousarray(values)
    shift = _checked_shift(shift, n_out, L)
    used = values[:, 0, :].copy() if shift is None and N > 0 else shift
    if values.nbytes <= slab_bytes:
        return (used,) + _moments4_call(values, N, L, n_out, shift, differences, None)
    # as pilot_statistics: one output at a time, a run of samples of ONE output is contiguous as it lies
    per_slab = max(int(slab_bytes) // max(L * 8, 1) // BLUEST_PILOT_CHUNK, 1) * BLUEST_PILOT_CHUNK
    outputs = []
    for n in range(n_out):
        total = None
        for start in range(0, N, per_slab):
            slab = values[n:n + 1, start:start + per_slab, :]
            part = _moments4_call(slab, slab.shape[1], L, 1, used[n:n + 1], differences, None)
            total = part if total is None else tuple(None if t is None else t + q for t, q in zip(total, part))
        outputs.append(total)
    return (used,) + tuple(None if parts[0] is None else np.concatenate(parts, axis=0) for parts in zip(*outputs))


def _central(N, first, s11):
    """the 1/N covariance of the shifted samples (the shift drops out): mu11 [n_out, L, L]"""
    a = first / N
    return s11 / N - a[:, :, None] * a[:, None, :]


def _difference_variance(N, tpow):
    """the 1/N variance of t, [n_out, L, L] (meaningful at i < j)"""
    return tpow[:, 1] / N - (tpow[:, 0] / N) ** 2


def pilot_standard_errors(N, first, s11, s21, s22, tpow=None):
    """(SE(C^) [n_out, L, L], SE(dV^) [n_out, L, L] or None without tpow) from the sums of pilot_fourth_moments over N samples, in
    float64.  C^_ij = mu11 is the 1/N estimate PilotMixin writes; with the unbiased s_ij = N / (N - 1) C^_ij and the central
    moments mu.. of the shifted samples,
        Var(s_ij) = mu22 / N - (N - 2) mu11^2 / (N (N - 1)) + mu20 mu02 / (N (N - 1)),    SE(C^_ij) = (N - 1) / N sqrt(max(Var, 0)),
    and for the difference variance, from the central moments mu2, mu4 of t,
        Var(s^2) = mu4 / N - (N - 3) mu2^2 / (N (N - 1)),                                 SE(dV^) = (N - 1) / N sqrt(max(Var, 0)).
    SE(dV^) is NaN outside i < j; N < 2 gives NaN everywhere."""
    first, s11, s21, s22 = (np.asarray(x, dtype=np.float64) for x in (first, s11, s21, s22))
    N = int(N)
    if N < 2:
        return np.full(s11.shape, np.nan), (None if tpow is None else np.full(s11.shape, np.nan))
    a, b = (first / N)[:, :, None], (first / N)[:, None, :]
    m11, m21, m22 = s11 / N, s21 / N, s22 / N
    diag = np.diagonal(m11, axis1=1, axis2=2)
    m20, m02 = diag[:, :, None], diag[:, None, :]
    ab = a * b
    mu11, mu20, mu02 = m11 - ab, m20 - a * a, m02 - b * b
    # (every term is grouped so that swapping i and j gives the same bits: the errors are symmetric as the estimates are)
    mu22 = m22 - 2 * (b * m21 + a * m21.transpose(0, 2, 1)) + (b * b * m20 + a * a * m02) + 4 * ab * m11 - 3 * ab * ab
    var = mu22 / N - (N - 2) * mu11 ** 2 / (N * (N - 1)) + mu20 * mu02 / (N * (N - 1))
    se_c = (N - 1) / N * np.sqrt(np.maximum(var, 0.0))
    if tpow is None:
        return se_c, None
    m1, m2, m3, m4 = (np.asarray(tpow, dtype=np.float64)[:, k] / N for k in range(4))
    mu2 = m2 - m1 * m1
    mu4 = m4 - 4 * m1 * m3 + 6 * m1 * m1 * m2 - 3 * m1 ** 4
    var = mu4 / N - (N - 3) * mu2 ** 2 / (N * (N - 1))
    se_d = (N - 1) / N * np.sqrt(np.maximum(var, 0.0))
    se_d[:, ~np.triu(np.ones(se_d.shape[1:], dtype=bool), 1)] = np.nan
    return se_c, se_d


def next_pilot_size(N, r, size, N_max):
    """the pilot size after N samples whose largest error-to-tolerance ratio is r > 1: the 1/sqrt(N) law with 10 % to spare, at
    most four times and at least one sample per rank more, a multiple of the communicator size, capped at N_max"""
    want = 4 * N if not math.isfinite(r) else min(4 * N, int(math.ceil(1.1 * N * r * r)))
    return min(N_max, next_divisible_number(max(N + size, want), size))


def tolerance_ratio(tol, se_c, se_d, C_hat, dV_hat, unknown, no_dV, linked):
    """the largest ratio of an error to what the tolerance allows over the estimated coupled entries of one output: SE(C^_ij)
    against tol sqrt(C^_ii C^_jj) where `unknown`, SE(dV^_ij) against tol dV^_ij at i < j where `no_dV` and `linked`; all [L, L].
    inf where an error that counts is NaN, 0.0 where nothing counts"""
    ratio = 0.0
    var = np.diagonal(C_hat)
    scale = np.sqrt(np.outer(var, var))
    use = unknown & (scale > 0)
    pairs = (no_dV & linked) & np.triu(np.ones(scale.shape, dtype=bool), 1) & (dV_hat > 0) & (scale > 0)
    for err, ref, mask in ((se_c, scale, use), (se_d, dV_hat, pairs)):
        if mask.any():
            r = err[mask] / (tol * ref[mask])
            ratio = max(ratio, float(np.inf if np.isnan(r).any() else r.max()))
    return ratio


class _GrowingPilot(object):
    """what PilotErrorsMixin and bluest_amd.field_pilot_errors.FieldPilotErrorsMixin share: the refusals, the growth loop, the
    errors it writes back, the report and the accessors.  A mix-in on top of it supplies
        _pilot_needs                      what a tolerance needs, for the refusal's message
        _pilot_unavailable()              why the GPU sums of the pilot are not there, or None
        _pilot_caps(ls, N, size)          (the largest pilot size, which cap binds: "samples" or "bytes")
        _pilot_round(ls, N, estimates)    rank 0: (SE(C^), SE(dV^), C^, dV^) [n_outputs, L, L] of the values kept; the last two
                                          only with `estimates`, else None
        _pilot_reset()                    forget what the rounds kept (extend it for state of its own)
        _pilot_reported(...)              the report (extend it for keys of its own)
    and the hooks of its bases through which a round draws what is missing and rank 0 keeps what was drawn."""
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message
    pilot_report = None
    _pilot_errors = None                 # (errors of C [n_outputs, M, M], errors of dV [n_outputs, M, M])
    _pilot_kept = None                   # rank 0, while the pilot runs: the values drawn so far
    _pilot_have = 0                      # every rank: how many samples the values kept on rank 0 hold

    def _pilot_tol(self):
        tol = self.params.get("covariance_estimation_tol")
        if tol is not None and not float(tol) > 0:
            raise ValueError("covariance_estimation_tol must be positive")
        return None if tol is None else float(tol)

    def _pilot_reset(self):
        self._pilot_kept, self._pilot_have = None, 0

    def _pilot_reported(self, samples, rounds, ratio, converged, cap):
        return dict(samples=samples, rounds=rounds, ratio=ratio, converged=converged)

    # ---- BLUEProblem's hooks ----------------------------------------------------------------------------------------------------
    def _init_inputs(self, C, costs):
        why = self._pilot_unavailable()
        if why is not None and self._pilot_tol() is not None:
            raise BLUESTError("covariance_estimation_tol needs %s: %s" % (self._pilot_needs, why))
        return super()._init_inputs(C, costs)

    def _init_from_datafile(self, datafile, costs):
        if self._pilot_tol() is not None:
            raise BLUESTError("covariance_estimation_tol needs pilot samples: a problem loaded from a model-graph file draws none")
        return super()._init_from_datafile(datafile, costs)

    def estimate_missing_covariances(self, N):
        """the bases' estimate_missing_covariances, then the standard errors of what it estimated; with
        params["covariance_estimation_tol"] the pilot grows from N samples until the errors meet the tolerance"""
        if self._pilot_unavailable() is not None:
            return super().estimate_missing_covariances(N)
        unknown = [cp.linked & np.isnan(cp.cov) for cp in self._coupling]
        ls = [int(l) for l in np.flatnonzero(np.logical_or.reduce(unknown).any(axis=1))]
        no_dV = [~np.isfinite(np.array(d, dtype=np.float64)) for d in self.dV]
        nan = lambda: np.full((self.n_outputs, self.M, self.M), np.nan)
        if len(ls) == 0:                                                # nothing to estimate: nothing has an error
            if self._pilot_errors is None:
                self._pilot_errors, self.pilot_report = (nan(), nan()), self._pilot_reported(0, 0, None, True, None)
            return
        self._pilot_errors = (nan(), nan())
        tol, comm = self._pilot_tol(), self.get_comm()
        size, N = comm.Get_size(), int(N)
        N_max, cap = self._pilot_caps(ls, N, size)
        before = ([cp.cov.copy() for cp in self._coupling], [np.array(d, dtype=np.float64) for d in self.dV])
        sub = np.ix_(ls, ls)
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
                    se_c, se_d, C_hat, dV_hat = self._pilot_round(ls, N, tol is not None)
                    ratio = 0.0 if tol is None else max(
                        tolerance_ratio(tol, se_c[n], se_d[n], C_hat[n], dV_hat[n], unknown[n][sub], no_dV[n][sub],
                                        self._coupling[n].linked[sub]) for n in range(self.n_outputs))
                    found = (se_c, se_d, ratio)
                se_c, se_d, ratio = comm.bcast(found, root=0)
                more = None
                if comm.Get_rank() == 0:                                # rank 0 decides
                    more = next_pilot_size(N, ratio, size, N_max) if tol is not None and ratio > 1 and N < N_max else N
                more = comm.bcast(more, root=0)
                if more == N:
                    break
                N = more
        finally:
            self._pilot_reset()
        where = np.ix_(range(self.n_outputs), ls, ls)
        self._pilot_errors[0][where] = se_c
        self._pilot_errors[1][where] = se_d
        for n in range(self.n_outputs):
            self._pilot_errors[0][n][~unknown[n]] = np.nan              # given, not estimated
            self._pilot_errors[1][n][~(no_dV[n] & np.triu(np.ones((self.M, self.M), dtype=bool), 1))] = np.nan
        converged = tol is None or ratio <= 1
        self.pilot_report = self._pilot_reported(N, rounds, float(ratio) if tol is not None else None, converged,
                                                 None if converged else cap)
        if not converged and comm.Get_rank() == 0:
            print("WARNING! The pilot estimates miss covariance_estimation_tol = %g after %d samples (largest error / tolerance: "
                  "%.3g). Raise covariance_estimation_max_%s." % (tol, N, ratio, cap))

    # ---- what was measured --------------------------------------------------------------------------------------------------------
    def _errors(self):
        if self._pilot_errors is None:
            why = self._pilot_unavailable() or "nothing was estimated from pilot samples (a problem loaded from a model-graph file?)"
            raise BLUESTError("no standard errors of the pilot estimates: " + why)
        return self._pilot_errors

    def get_covariance_errors(self):
        """per output M x M, symmetric: the standard error of every covariance entry that was estimated from the pilot samples, NaN
        where the entry was given.  An entry the |rho| < 1e-7 rule set to 0 keeps the error of its estimate.  The errors refer to the
        estimates BEFORE any SPD projection (project_covariances moves the entries afterwards)."""
        return [e.copy() for e in self._errors()[0]]

    def get_covariance_error(self, n=0):
        return self._errors()[0][n].copy()

    def get_mlmc_variance_errors(self):
        """per output M x M, at i < j: the standard error of every MLMC difference variance that was estimated, NaN elsewhere"""
        return [e.copy() for e in self._errors()[1]]

    def get_mlmc_variance_error(self, n=0):
        return self._errors()[1][n].copy()


class PilotErrorsMixin(_GrowingPilot):
    _pilot_needs = "the fourth moments of scalar pilot samples"

    def _pilot_unavailable(self):
        """why the sums do not come from bluest_pilot_stats, or None"""
        from .fields import FieldOutputsMixin
        if isinstance(self, FieldOutputsMixin):
            return "FieldOutputsMixin takes its sums from bluest_field_stats"
        if type(self).get_models_inner_products is not BLUEProblem.get_models_inner_products:
            return "inner products written in Python are summed on the host"
        return None

    def _pilot_caps(self, ls, N, size):
        return max(N, int(self.params.get("covariance_estimation_max_samples", 64 * N))), "samples"

    # ---- PilotMixin's hooks: a round draws what is missing, rank 0 keeps what was drawn [n_outputs, N, L] --------------------------
    def _pilot_values(self, ls, N):
        return super()._pilot_values(ls, N - self._pilot_have)

    def _pilot_gathered(self, ls, values):
        if self._pilot_kept is not None:
            values = np.concatenate([self._pilot_kept, values], axis=1)                   # round-major, then in rank order
        self._pilot_kept = values
        return values

    def _pilot_round(self, ls, N, estimates):
        _, first, s11, s21, s22, tpow = pilot_fourth_moments(self._pilot_kept, differences=True)
        se_c, se_d = pilot_standard_errors(N, first, s11, s21, s22, tpow)
        if not estimates:
            return se_c, se_d, None, None
        return se_c, se_d, _central(N, first, s11), _difference_variance(N, tpow)

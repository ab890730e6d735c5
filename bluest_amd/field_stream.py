"""
A field group's samples streamed through resumable sums and moments: a sampled group never has to exist as one array [N, L, d].

The order contract of include/bluest_hip.h, Parts 11, 12 and 15, cuts a segment into chunks of 128 rows, gives chunk c to lane
c mod 64, which adds its chunks in ascending order from +0.0, and joins the lanes in a tree.  The running state of a segment is
therefore the 64 lane partials per output value, the first row and at most 127 rows of an unfinished chunk, and a segment delivered
in pieces of any sizes gives the bits of the one-shot calls (Part 19; csrc/field_accum.hip).  There is no CPU path.

FieldAccumulator(L, d, coef=None)    a context manager around one bluest_field_accum handle.
    update(values)      [n, L, d] float64, a numpy array or a CUDA tensor (read where it lies, on the tensor's current stream); n may
                        be 0.  The call returns when the rows have been taken: the batch may be freed.
    finish()            (N, sums [L, d], zsum [d] or None, zsq [d] or None): the bits of field_group_sums([whole])[0] and, with
                        coef [L], of field_weighted_moments([whole], coef)[0] on the concatenated rows.
    close()             frees the device state; also at the end of the `with` block.

StreamedFieldsMixin   opt-in, listed first:

    class MyProblem(StreamedFieldsMixin, FieldErrorsMixin, FieldOutputsMixin, SamplingMixin, BLUEProblem): ...
    p = MyProblem(M, ..., field_stream_bytes=256 << 20)

    A group of m_g joint samples of L models is STREAMED when m_g * L * sum(widths) * 8 >= field_stream_bytes (0: every group):
    its batches go one by one -- shaped, checked, resampled and mapped exactly as draw_field_values does, with the same sampler /
    evaluate calls -- into one accumulator per output, and only its sums [L, d_n] and (N, zsum, zsq) are kept.  solve(),
    variance_test(), the estimators of MFMC / MLMC / MC and FieldErrorsMixin's field_sample_moments keep their bits: the flushes
    fall where they fell, and a streamed group enters a flush's field_group_sums call as a segment of ONE sample, its sums,
    which passes through unchanged (x + 0.0 is x, the class and lane trees add +0.0, and a sum that started from +0.0 is never
    -0.0).  Below the threshold the mix-in behaves as its bases.
    Refused with BLUESTError where a group reaches the threshold: a communicator of more than one rank (the ranks' shares join at
    rank boundaries, not in arrival order), and FieldCovariancesMixin among the bases (Part 16 is not resumable).
"""
import ctypes

import numpy as np

from . import _lib, fields
from .blue_models import BLUEST_MAX_MODELS
from .estimator import SLAB_BYTES, sampled_columns
from .field_errors import variance_of
from .sap import BLUESTError

FIELD_STREAM_BYTES = 256 << 20


class FieldAccumulator(object):
    def __init__(self, L, d, coef=None, slab_bytes=SLAB_BYTES):
        """`slab_bytes`: a host batch goes to the GPU in slabs of whole chunks of at most this size; the result does not depend
        on it.  The device state is made with the first update or finish."""
        L, d = int(L), int(d)
        if L < 1 or L > BLUEST_MAX_MODELS:
            raise ValueError("L must lie in 1..%d" % BLUEST_MAX_MODELS)
        if d < 1:
            raise ValueError("d must be at least 1")
        if coef is not None:
            coef = np.ascontiguousarray(np.asarray(coef, dtype=np.float64))
            if coef.shape != (L,):
                raise ValueError("coef must have one entry per model: shape [%d]" % L)
            if not np.all(np.isfinite(coef)):
                raise ValueError("coef must be finite")
        self.L, self.d, self.coef, self.slab_bytes = L, d, coef, slab_bytes
        self._handle, self._closed = None, False

    def _open(self):
        if self._closed:
            raise ValueError("the accumulator is closed")
        if self._handle is None:
            handle = ctypes.c_void_p()
            _lib.check(_lib.lib().bluest_field_accum_create(self.L, self.d, _lib.ptr(self.coef), ctypes.byref(handle), None))
            self._handle = handle
        return self._handle

    def update(self, values):
        v = fields._segment(values, "values")
        if tuple(int(x) for x in v.shape[1:]) != (self.L, self.d):
            raise ValueError("values must have the shape [n, %d, %d]" % (self.L, self.d))
        handle = self._open()
        stream = fields._stream_of(v) if hasattr(v, "data_ptr") else None
        n = int(v.shape[0])
        with _lib.staging_budget(self.slab_bytes):
            _lib.check(_lib.lib().bluest_field_accum_update(handle, n, _lib.ptr(v) if n > 0 else None, stream))

    def finish(self):
        handle = self._open()
        count = ctypes.c_int64(0)
        sums = np.empty((self.L, self.d))
        zsum, zsq = (np.empty(self.d), np.empty(self.d)) if self.coef is not None else (None, None)
        _lib.check(_lib.lib().bluest_field_accum_finish(handle, ctypes.byref(count), _lib.ptr(sums), _lib.ptr(zsum), _lib.ptr(zsq), None))
        return int(count.value), sums, zsum, zsq

    def info(self):
        """bluest_field_accum_info: rows taken, chunks carried, rows in the tail, device allocations, launches of the sum kernel,
        launches of a moment kernel, device bytes held, finished"""
        out = np.zeros(8, dtype=np.int64)
        _lib.check(_lib.lib().bluest_field_accum_info(self._open(), out.ctypes.data_as(_lib.c_i64p)))
        return out.tolist()

    def close(self):
        if self._handle is not None:
            _lib.lib().bluest_field_accum_destroy(self._handle)
            self._handle = None
        self._closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

    def __del__(self):
        try:
            self.close()
        except Exception:                                               # (the library may be gone at interpreter exit)
            pass


def stream_group(problem, ls, N, widths, coefs=None):
    """the N joint samples of the models `ls` drawn batch by batch into one accumulator per output: per output
    (N, sums [L, d_n], zsum, zsq), the last two None without coefs[n]"""
    L = len(ls)
    accs = [FieldAccumulator(L, widths[n], coef=None if coefs is None else coefs[n]) for n in range(problem.n_outputs)]
    try:
        for batch in fields.field_batches(problem, ls, N, widths, device_ok=True):
            for n, acc in enumerate(accs):
                acc.update(batch[n])
            del batch
        return [acc.finish() for acc in accs]
    finally:
        for acc in accs:
            acc.close()


class StreamedFieldsMixin(object):
    def __init__(self, *args, field_stream_bytes=FIELD_STREAM_BYTES, **kw):
        self.field_stream_bytes = int(field_stream_bytes)
        if self.field_stream_bytes < 0:
            raise ValueError("field_stream_bytes must not be negative")
        super().__init__(*args, **kw)

    def _field_streamed(self, m, L, widths):
        return int(m) > 0 and int(m) * L * sum(widths) * 8 >= self.field_stream_bytes

    def _field_stream_refusals(self, covariances):
        if self.get_comm().Get_size() > 1:
            raise BLUESTError("a group reaches field_stream_bytes, and a streamed group cannot be drawn by more than one rank: the "
                              "ranks' shares join at rank boundaries, not in the order they arrive in")
        if covariances:
            from .field_covariances import FieldCovariancesMixin
            if isinstance(self, FieldCovariancesMixin):
                raise BLUESTError("a group reaches field_stream_bytes, and FieldCovariancesMixin needs the group's samples held: the "
                                  "second moments of a field (bluest_field_group_moments) are not resumable")

    # ---- one group ----------------------------------------------------------------------------------------------------------------
    def _group_sums(self, ls, N):
        ws, is_field = self._field_weights()
        widths = [len(w) for w in ws]
        if not self._field_streamed(N, len(ls), widths):
            return super()._group_sums(ls, N)
        self._check_field_width(len(ls))
        self._field_stream_refusals(covariances=False)
        got = stream_group(self, ls, N, widths)
        return [[self._plain(got[n][1][i], is_field[n]) for i in range(len(ls))] for n in range(self.n_outputs)]

    # ---- whole estimators -------------------------------------------------------------------------------------------------------------
    def _sample_estimators(self, n_rep):
        """FieldOutputsMixin._sample_estimators: the same draws, the same flushes, the same field_group_sums call per output and
        flush.  Where a group streams, what is refused is refused here, before anything is drawn or checked"""
        widths = [len(w) for w in self._field_weights()[0]]
        if any(self._field_streamed(m, len(ls), widths) for _, ls, _, m in sampled_columns(self.MOSAP_output)):
            self._field_stream_refusals(covariances=True)
        return super()._sample_estimators(n_rep)

    def _field_group_values(self, col, widths):
        """a streamed group is never held: it stands in the flush as one row, its sums, and a collecting solve() gets its
        (N, variance of z) from the accumulators"""
        g, ls, c, m = col
        if not self._field_streamed(m, len(ls), widths):
            return super()._field_group_values(col, widths)
        collecting = getattr(self, "_collecting_fields", None)
        coefs = None
        if collecting is not None:
            W = self._blue_weights()[0]
            coefs = [W[n, c:c + len(ls)] for n in range(self.n_outputs)]
        got = stream_group(self, ls, m, widths, coefs)
        if collecting is not None:
            for n, (N, _, zsum, zsq) in enumerate(got):
                collecting[n][g] = (N, variance_of(N, zsum, zsq))
        return [s[1][None] for s in got], False

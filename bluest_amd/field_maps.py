"""
Fields on per-model meshes: sparse maps to a space all models of an output share, on the GPU (include/bluest_hip.h, Part 18;
csrc/field_map.hip).  Every field call of this package takes the values of a model group as ONE array [N, L, d]; the models of a
multilevel or multi-fidelity problem deliver d_l nodal values each.  Point evaluation, prolongation to the finest mesh,
restriction to an observation grid and evaluation at quadrature points are all a sparse matrix B_l (q x d_l); the reference's
field example (examples/multi_output_example.py) applies two point evaluations on the host inside `evaluate` because nothing
downstream of it can combine vectors of different lengths.

FieldOperator(matrix, shape=None)
    a sparse q x d matrix: from a CSR triple (indptr, indices, data) with shape=(q, d) -- or, as one object, the pair (triple,
    (q, d)) --, from any object with .tocsr() (scipy is used only if the caller brings such an object), or from a dense 2-D
    array, row by row with its zeros left out.  The entries of a row keep their stored order -- Part 18 adds them in that
    order -- and a column may occur twice.  .shape, .nnz, .csr().  The device copy is made at the first map_fields call that
    uses the operator and goes when the object is collected.
map_fields(values, operators, slab_bytes=SLAB_BYTES)
    values: L arrays [N, d_l], numpy or float64 CUDA tensors, mixed; operators: L entries, a FieldOperator or None (identity,
    d_l == q).  -> [N, L, q], out[s, l] = B_l values[l][s]: a CUDA tensor if any input is one, else a numpy array.  The order
    of every operation is fixed (Part 18): the same bits from host or device memory and under any `slab_bytes`.  No CPU path.

MappedFieldsMixin   opt-in, listed first, in front of the other field mix-ins where those are wanted:

    class MyProblem(MappedFieldsMixin, FieldOutputsMixin, SamplingMixin, PilotMixin, BLUEProblem):
        def output_operators(self): return [None, [None, P1, P2]]       # per output: None = as without this mix-in, or M entries,
                                                                        # one per model: None (identity) or what FieldOperator takes
        def output_weights(self):   return [None, w]                    # q_n weights: they live in the COMMON space
        def evaluate(self, ls, samples, N=1): ...                       # Ps[n][i]: the d_{n, ls[i]} components of model ls[i] itself,
                                                                        # [d] for a batch of one or [N2, d], host or CUDA

    Every batch is mapped as it arrives, after the finiteness check on the RAW values, so resampling and the whole sequence of
    sampler / evaluate calls are those of the unmapped problem; the raw values live for one batch and CUDA batches stay on the
    device.  Everything downstream receives [N2, L, q_n] and is unchanged: pilot statistics, the MLMC differences
    B_i y_i - B_j y_j, group sums, estimators, and the hooks FieldErrorsMixin, FieldCovariancesMixin and FieldPilotErrorsMixin
    use.  solve() returns mus[n] in the common space [q_n]; C and dV are in the inner product sum_r w_r (B_i y_i)_r (B_j y_j)_r,
    dV from the explicit differences of the mapped fields.  With the same B (evaluation at quadrature points) for every model
    and w the quadrature weights this is the non-diagonal inner product a^T B^T diag(w) B b, which output_weights() alone cannot
    express.  With an MPI communicator each rank maps what it drew, before the gather: rank 0 receives mapped values.
    Refused (BLUESTError, when the problem is constructed): inner products written in Python together with operators, a list of
    operators whose length is not M, operators of one output with different q, len(output_weights()[n]) != q_n, an operator on an
    output whose weight is None.  An identity entry stands for d == q: a model that delivers another width is refused by the
    width check of the first batch, as any wrong width is.  Sample files and reorder_graph_nodes stay refused.
"""
import ctypes

import numpy as np

from . import _lib
from .blue_models import BLUEProblem
from .estimator import SLAB_BYTES
from .fields import FieldOutputsMixin, _stream_of
from .sap import BLUESTError

BLUEST_FIELD_MAP_STRIP = 512         # include/bluest_hip.h, Part 18


class FieldOperator(object):
    def __init__(self, matrix, shape=None):
        if isinstance(matrix, FieldOperator):
            indptr, indices, data = matrix.csr()
            shape = matrix.shape
        elif hasattr(matrix, "tocsr"):
            m = matrix.tocsr()
            indptr, indices, data, shape = m.indptr, m.indices, m.data, m.shape
        elif isinstance(matrix, (tuple, list)) and len(matrix) == 3 and shape is not None:
            indptr, indices, data = matrix
        elif (isinstance(matrix, tuple) and len(matrix) == 2 and shape is None and isinstance(matrix[0], (tuple, list))
              and len(matrix[0]) == 3 and np.ndim(matrix[0][0]) == 1 and np.shape(matrix[1]) == (2,)):
            (indptr, indices, data), shape = matrix                     # ((indptr, indices, data), (q, d)): the triple as ONE object
        else:
            dense = np.asarray(matrix, dtype=np.float64)
            if dense.ndim != 2:
                raise ValueError("a FieldOperator is built from (indptr, indices, data) with shape=(q, d), from an object with .tocsr() "
                                 "or from a dense 2-D array")
            keep = dense != 0.0
            indptr = np.concatenate([[0], np.cumsum(keep.sum(axis=1))])
            indices = np.nonzero(keep)[1]                               # row-major: row by row, columns ascending
            data = dense[keep]
            shape = dense.shape
        q, d = (int(x) for x in shape)
        indptr = np.array(indptr, dtype=np.int64).reshape(-1)
        data = np.array(data, dtype=np.float64).reshape(-1)
        wide = np.array(indices, dtype=np.int64).reshape(-1)
        if q < 1 or d < 1 or d > 2**31 - 1:
            raise ValueError("shape=(%d, %d): an operator has at least one row and one column and at most 2^31 - 1 columns" % (q, d))
        if indptr.shape != (q + 1,) or indptr[0] != 0 or np.any(np.diff(indptr) < 0):
            raise ValueError("indptr must have q + 1 = %d entries that start at 0 and do not decrease" % (q + 1))
        nnz = int(indptr[-1])
        if nnz > 2**31 - 1 or wide.shape != (nnz,) or data.shape != (nnz,):
            raise ValueError("indices and data must have indptr[-1] = %d entries each (at most 2^31 - 1)" % nnz)
        if nnz and (wide.min() < 0 or wide.max() >= d):
            raise ValueError("a column index lies outside 0..%d" % (d - 1))
        if not np.all(np.isfinite(data)):
            raise ValueError("the coefficients must be finite")
        self.shape, self.nnz = (q, d), nnz
        self._csr = (indptr, wide.astype(np.int32), data)
        for a in self._csr:
            a.setflags(write=False)
        self._handle = None

    def csr(self):
        """(indptr int64 [q + 1], indices int32 [nnz], data float64 [nnz]) as stored: read-only"""
        return self._csr

    def handle(self):
        """the bluest_field_op_t of this operator; made, and the matrix uploaded, at the first call"""
        if self._handle is None:
            h = ctypes.c_void_p()
            indptr, indices, data = self._csr
            _lib.check(_lib.lib().bluest_field_op_create(self.shape[0], self.shape[1], _lib.ptr(indptr), _lib.ptr(indices), _lib.ptr(data),
                                                         ctypes.byref(h)))
            self._handle = h
        return self._handle

    def __del__(self):
        h, self._handle = getattr(self, "_handle", None), None
        if h is not None:
            try:
                _lib.lib().bluest_field_op_destroy(h)
            except Exception:                                           # the interpreter is going away
                pass


def _samples(v, l):
    """values[l] as a contiguous float64 [N, d] numpy array or CUDA tensor"""
    if hasattr(v, "data_ptr"):
        import torch
        if v.dim() != 2 or v.dtype != torch.float64:
            raise ValueError("values[%d] must be a float64 array of shape [N, d]" % l)
        if v.is_cuda:
            return v.contiguous()
        v = v.numpy()
    v = np.ascontiguousarray(np.asarray(v, dtype=np.float64))
    if v.ndim != 2:
        raise ValueError("values[%d] must be a float64 array of shape [N, d]" % l)
    return v


def map_fields(values, operators, slab_bytes=SLAB_BYTES):
    """[N, L, q] with out[s, l] = operators[l] applied to values[l][s] (None: the identity), bit for bit by the rule of Part 18;
    a CUDA tensor if any of the values is one, else a numpy array.  `slab_bytes`: host arrays go to the GPU and back in runs of
    whole samples of at most this size; the result does not depend on it."""
    L = len(values)
    if L < 1 or len(operators) != L:
        raise ValueError("map_fields needs one operator entry (or None) per array of values, and at least one")
    keep = [_samples(v, l) for l, v in enumerate(values)]
    for op in operators:
        if op is not None and not isinstance(op, FieldOperator):
            raise ValueError("an operator entry is a FieldOperator or None")
    qs = set(op.shape[0] for op in operators if op is not None)
    if len(qs) > 1:
        raise ValueError("the operators of one call must have the same number of rows, not %s" % sorted(qs))
    q = qs.pop() if qs else int(keep[0].shape[1])
    N = int(keep[0].shape[0])
    for l, (v, op) in enumerate(zip(keep, operators)):
        need = q if op is None else op.shape[1]
        if int(v.shape[0]) != N or int(v.shape[1]) != need:
            raise ValueError("values[%d] has shape %s: %s needs [%d, %d]" % (l, tuple(v.shape), "the identity" if op is None else
                                                                             "its operator", N, need))
    first = next((v for v in keep if hasattr(v, "data_ptr")), None)
    if first is not None:
        import torch
        out = torch.empty((N, L, q), dtype=torch.float64, device=first.device)
        stream = _stream_of(first)
    else:
        out, stream = np.empty((N, L, q)), None
    handles = (ctypes.c_void_p * L)(*[None if op is None else op.handle() for op in operators])
    ptrs = (ctypes.c_void_p * L)(*[_lib.ptr(v) if N > 0 else None for v in keep])
    with _lib.staging_budget(slab_bytes):
        _lib.check(_lib.lib().bluest_field_map(N, L, q, ctypes.cast(handles, ctypes.c_void_p), ctypes.cast(ptrs, ctypes.c_void_p),
                                               _lib.ptr(out) if N > 0 else None, stream))
    return out


class MappedFieldsMixin(object):
    reorder_graph_nodes = reorder_all_graph_nodes = BLUEProblem._out_of_scope      # named here so that they refuse with a message
    _mapped_ops = None

    # ---- what the user declares -----------------------------------------------------------------------------------------------------
    def output_operators(self):
        """per output: None (the output is what it is without this mix-in), or M entries, one per model: None for the identity, a
        FieldOperator, or anything FieldOperator accepts"""
        return [None] * self.n_outputs

    def _mapped_operators(self):
        """per output None, or the M entries as None / FieldOperator: checked against output_weights() once, then kept (an
        operator is uploaded once)"""
        if self._mapped_ops is not None:
            return self._mapped_ops
        if not isinstance(self, FieldOutputsMixin):
            raise BLUESTError("MappedFieldsMixin maps the batches FieldOutputsMixin draws: FieldOutputsMixin is not among the bases")
        declared = list(self.output_operators())
        if len(declared) != self.n_outputs:
            raise BLUESTError("output_operators() must have one entry per output (%d), not %d" % (self.n_outputs, len(declared)))
        if (any(ops is not None for ops in declared)
                and type(self).get_models_inner_products is not FieldOutputsMixin.get_models_inner_products):
            raise BLUESTError("output_operators() needs the inner products of output_weights(): inner products written in Python "
                              "cannot be combined with operators")
        weights = list(self.output_weights())
        ws, _ = self._field_weights()
        out = []
        for n, ops in enumerate(declared):
            if ops is None:
                out.append(None)
                continue
            if weights[n] is None:
                raise BLUESTError("output %d is a number (its weight is None): it takes no operators" % n)
            ops = list(ops)
            if len(ops) != self.M:
                raise BLUESTError("output_operators()[%d] must have one entry per model (%d), not %d" % (n, self.M, len(ops)))
            try:
                ops = [op if op is None or isinstance(op, FieldOperator) else FieldOperator(op) for op in ops]
            except ValueError as e:
                raise BLUESTError("output_operators()[%d]: %s" % (n, e))
            qs = sorted(set(op.shape[0] for op in ops if op is not None))
            if len(qs) > 1:
                raise BLUESTError("the operators of output %d map into spaces of different sizes %s" % (n, qs))
            if qs and qs[0] != len(ws[n]):
                raise BLUESTError("output_weights()[%d] has %d entries: the weights live in the common space of the operators, q = %d"
                                  % (n, len(ws[n]), qs[0]))
            out.append(ops)
        self._mapped_ops = out
        return out

    # ---- BLUEProblem's hooks: the declarations are checked before anything is drawn ------------------------------------------------
    def _init_inputs(self, C, costs):
        self._mapped_operators()
        return super()._init_inputs(C, costs)

    def _init_from_datafile(self, datafile, costs):
        self._mapped_operators()
        return super()._init_from_datafile(datafile, costs)

    # ---- bluest_amd.fields.draw_field_values' hook ----------------------------------------------------------------------------------
    def _field_batch_hook(self, ls):
        """per output None, or (the widths d_{n, l} of the models `ls` themselves, a function that takes their raw batches --
        len(ls) arrays [N2, d], host or CUDA -- to [N2, len(ls), q_n])"""
        ws, _ = self._field_weights()
        hooks = []
        for n, ops in enumerate(self._mapped_operators()):
            if ops is None:
                hooks.append(None)
                continue
            mine = [ops[l] for l in ls]
            hooks.append(([len(ws[n]) if op is None else op.shape[1] for op in mine], lambda raws, mine=mine: map_fields(raws, mine)))
        return hooks

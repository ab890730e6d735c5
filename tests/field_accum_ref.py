"""numpy restatement of the STREAMED order of include/bluest_hip.h, Part 19 (bluest_field_accum_*): the rows of one segment arrive in
pieces, wait in a tail of fewer than 128 rows, leave it chunk by chunk with the chunk values of fields_ref / field_moments_ref,
are carried into 64 lane partials by c mod 64 update by update, and finish runs the tail as the last, short chunk and the tree
over the lanes.  Nothing here looks at the whole segment, so its agreement with the one-shot restatements
(fields_ref.segment_sums, field_moments_ref.segment_moments) on the concatenation is the equality argument of Part 19, checked
without a GPU.  StubAccumulator stands in for bluest_amd.field_stream.FieldAccumulator in the host tests."""
import numpy as np

import field_moments_ref as mref
import gsums_ref
from gsums_ref import CHUNK, LANES


def tree(p):
    """for off = 32 .. 1, lane l < off takes p[l] + p[l + off]; the result is lane 0's"""
    p = list(p)
    off = LANES // 2
    while off > 0:
        for l in range(off):
            p[l] = p[l] + p[l + off]
        off //= 2
    return p[0]


class FieldAccumRef(object):
    def __init__(self, L, d, coef=None, exact_products=False):
        self.L, self.d, self.exact = int(L), int(d), exact_products
        self.coef = None if coef is None else np.asarray(coef, dtype=np.float64)
        self.lanes_s = [np.zeros((self.L, self.d)) for _ in range(LANES)]
        self.lanes_m = [np.zeros((2, self.d)) for _ in range(LANES)]
        self.first = None
        self.tail = np.zeros((0, self.L, self.d))
        self.count, self.chunks_done, self.finished = 0, 0, False
        self.moment_chunks = 0

    def _chunk(self, block):
        """([L, d], [2, d] or None): the values of a chunk of at most 128 rows -- steps 1 and 2 of Part 11, and Part 15's with
        the segment's first row as the shift"""
        rows = block.shape[0]
        s = gsums_ref.chunk_sums(block.reshape(1, rows, self.L * self.d))[0].reshape(self.L, self.d)
        if self.coef is None:
            return s, None
        with np.errstate(invalid="ignore", over="ignore"):
            z = mref.chains(np.concatenate([self.first[None], block]), self.coef, self.exact)[1:]      # z of the rows, shifted by `first`
            m = np.stack([gsums_ref.chunk_sums(z[None])[0], mref.chunk_squares(z, self.exact)])
        self.moment_chunks += 1
        return s, m

    def _carry(self, chunks):
        """the chunks of one update have the global numbers c0 .. c0 + nc - 1: lane l takes its partial, adds the values of its
        chunks in ascending order and stores it"""
        c0, nc = self.chunks_done, len(chunks)
        for i in range(min(nc, LANES)):
            lane = (c0 + i) % LANES
            acc_s, acc_m = self.lanes_s[lane], self.lanes_m[lane]
            for k in range(i, nc, LANES):
                acc_s = acc_s + chunks[k][0]
                if self.coef is not None:
                    acc_m = acc_m + chunks[k][1]
            self.lanes_s[lane], self.lanes_m[lane] = acc_s, acc_m
        self.chunks_done += nc

    def update(self, values):
        assert not self.finished
        v = np.asarray(values.cpu().numpy() if hasattr(values, "data_ptr") else values, dtype=np.float64)
        assert v.ndim == 3 and v.shape[1:] == (self.L, self.d)
        if v.shape[0] == 0:
            return
        if self.count == 0:
            self.first = v[0].copy()
        rows = np.concatenate([self.tail, v])                           # (at most 127 rows in front: the tail's chunk is completed)
        whole = rows.shape[0] // CHUNK
        with np.errstate(invalid="ignore", over="ignore"):
            self._carry([self._chunk(rows[k * CHUNK:(k + 1) * CHUNK]) for k in range(whole)])
        self.tail = rows[whole * CHUNK:].copy()
        self.count += v.shape[0]

    def finish(self):
        assert not self.finished
        with np.errstate(invalid="ignore", over="ignore"):
            if self.tail.shape[0] > 0:
                self._carry([self._chunk(self.tail)])
                self.tail = self.tail[:0]
            self.finished = True
            sums = tree(self.lanes_s)
            if self.coef is None:
                return self.count, sums, None, None
            m = tree(self.lanes_m)
        return self.count, sums, m[0], m[1]


class StubAccumulator(object):
    """bluest_amd.field_stream.FieldAccumulator with the restatement in place of the device; `made` keeps every instance"""
    made = []

    def __init__(self, L, d, coef=None, slab_bytes=None):
        self.ref = FieldAccumRef(L, d, coef)
        self.updates, self.closed = [], False
        StubAccumulator.made.append(self)

    def update(self, values):
        self.updates.append(int(values.shape[0]))
        self.ref.update(values)

    def finish(self):
        return self.ref.finish()

    def close(self):
        self.closed = True

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.close()
        return False

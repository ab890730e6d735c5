"""
Wall time of bluest_amd.field_maps.map_fields on device-resident values, against the torch expression a user would write today
and against fields.field_group_sums on the same output bytes (the bandwidth yardstick: one pass over [N, L, q]):

    python tools/field_map_bench.py [--out FILE]    # on the GPU machine; writes profiles/field_map_bench.txt

  shapes   prolongation  bilinear interpolation of 17^2, 33^2 and 65^2 nodes onto 129^2 (q = 16641, 4 entries per row), model 0 on
                         the fine grid itself (identity), N = 1000
           linear maps   N = 100, L = 3, d = 25000, 50000 and 100000 onto q = 100000, 3 entries per row
           dense rows    N = 10000, L = 8, q = 16 rows over all of d = 10000 columns: the long-row launch shape
  torch    per model torch.sparse.mm of a float64 CSR tensor with the transposed values, transposed back, then torch.stack over
           the models (an identity model goes into the stack as it is) and one synchronise; where torch.sparse.mm does not run on
           this build: index_select + multiply + sum over the entries of a row
Each call is timed REPEAT times after a warm-up, the three alternating.  map_fields is synchronous and returns a device tensor, as
the torch expression does; field_group_sums returns host arrays.  No ratio is fixed in advance; the file records what was measured.
"""
import os
import sys
import time

import numpy as np

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
REPEAT = 9


def interpolation_1d(n_from, n_to):
    """(first column [n_to], weights [n_to, 2]) of linear interpolation between equally spaced nodes"""
    x = np.arange(n_to) / (n_to - 1) * (n_from - 1)
    j = np.minimum(np.floor(x).astype(np.int64), n_from - 2)
    t = x - j
    return j, np.stack([1.0 - t, t], axis=1)


def bilinear(n_from, n_to):
    """CSR (n_to^2 x n_from^2) of bilinear interpolation, 4 entries per row"""
    j, w = interpolation_1d(n_from, n_to)
    cols = ((j[:, None, None, None] + np.arange(2)[None, None, :, None]) * n_from + (j[None, :, None, None] + np.arange(2)[None, None, None, :]))
    data = w[:, None, :, None] * w[None, :, None, :]
    q = n_to * n_to
    return np.arange(q + 1) * 4, cols.reshape(-1).astype(np.int32), data.reshape(-1), (q, n_from * n_from)


def three_point(d, q):
    """CSR (q x d): row r takes the columns around r d / q with the weights 1/4, 1/2, 1/4"""
    c = np.clip((np.arange(q) * d) // q, 1, d - 2)
    cols = c[:, None] + np.arange(-1, 2)[None, :]
    return np.arange(q + 1) * 3, cols.reshape(-1).astype(np.int32), np.tile([0.25, 0.5, 0.25], q), (q, d)


def dense_rows(q, d, seed):
    rng = np.random.RandomState(seed)
    return np.arange(q + 1) * d, np.tile(np.arange(d, dtype=np.int32), q), rng.uniform(-1.0, 1.0, q * d) / d, (q, d)


SHAPES = [
    ("prolongation onto 129^2", 1000, [None, bilinear(65, 129), bilinear(33, 129), bilinear(17, 129)]),
    ("3-point linear maps onto q = 100000", 100, [three_point(d, 100000) for d in (25000, 50000, 100000)]),
    ("dense rows, q = 16 over d = 10000", 10000, [dense_rows(16, 10000, l) for l in range(8)]),
]


def timed(fn):
    t0 = time.perf_counter()
    fn()
    return time.perf_counter() - t0


def summary(ts):
    return float(np.median(ts)) * 1e3, min(ts) * 1e3, max(ts) * 1e3


def main():
    import torch
    from bluest_amd import _lib, field_maps, fields
    assert torch.cuda.is_available()
    out = sys.argv[sys.argv.index("--out") + 1] if "--out" in sys.argv else os.path.join(ROOT, "profiles", "field_map_bench.txt")
    lines = ["# bluest_field_map on %s (BLUEST_FIELD_MAP_STRIP = %d); values in device memory, float64; wall time of one" % (_lib.device_name(), field_maps.BLUEST_FIELD_MAP_STRIP),
             "# synchronous call, median (and range) of %d after a warm-up, the calls alternating (tools/field_map_bench.py)." % REPEAT,
             "# bytes: 8 N (sum of d_l + L q), the values read and written once; the operators are not counted.  torch: per model",
             "# torch.sparse.mm(B_csr, y.T).T (or, where noted, the fall-back), torch.stack over the models, one synchronise.",
             "# field_group_sums: one pass over the mapped [N, L, q], its sums copied to the host.  Clocks: as the machine had them."]
    for name, N, csrs in SHAPES:
        L = len(csrs)
        q = next(c[3][0] for c in csrs if c is not None)
        ds = [q if c is None else c[3][1] for c in csrs]
        ops = [None if c is None else field_maps.FieldOperator(c[:3], shape=c[3]) for c in csrs]
        torch.manual_seed(N)
        values = [torch.randn(N, d, dtype=torch.float64, device="cuda") for d in ds]
        nbytes = 8 * N * (sum(ds) + L * q)
        how = "torch.sparse.mm"
        try:
            sparse = [None if c is None else torch.sparse_csr_tensor(torch.from_numpy(c[0]).cuda(), torch.from_numpy(c[1].astype(np.int64)).cuda(),
                                                                       torch.from_numpy(c[2]).cuda(), size=c[3], dtype=torch.float64) for c in csrs]

            def torch_map():
                res = torch.stack([v if B is None else torch.sparse.mm(B, v.T).T for v, B in zip(values, sparse)], dim=1)
                torch.cuda.synchronize()
                return res
            torch_map()
        except Exception as e:                                          # this build has no float64 CSR product
            how = "index_select + multiply + sum (torch.sparse.mm: %s)" % type(e).__name__
            gathered = [None if c is None else (torch.from_numpy(c[1].astype(np.int64)).cuda(), torch.from_numpy(c[2]).cuda().view(c[3][0], -1)) for c in csrs]

            def torch_map():
                res = torch.stack([v if g is None else (v.index_select(1, g[0]).view(N, g[1].shape[0], -1) * g[1]).sum(-1)
                                   for v, g in zip(values, gathered)], dim=1)
                torch.cuda.synchronize()
                return res
            torch_map()
        ours = lambda: field_maps.map_fields(values, ops)
        mapped = ours()
        sums = lambda: fields.field_group_sums([mapped])
        sums()
        want = torch_map()
        agree = float((mapped - want).abs().max() / want.abs().max())
        del want
        t_ours, t_torch, t_sums = [], [], []
        for _ in range(REPEAT):
            t_ours.append(timed(ours))
            t_torch.append(timed(torch_map))
            t_sums.append(timed(sums))
        m_ours, m_torch, m_sums = summary(t_ours), summary(t_torch), summary(t_sums)
        lines += ["", "%s: N = %d, L = %d, q = %d, d = %s, nnz = %s: %.1f MB of values in and out, %.1f MB of them out"
                  % (name, N, L, q, ds, [0 if c is None else len(c[1]) for c in csrs], nbytes / 1e6, 8 * N * L * q / 1e6),
                  "  map_fields                        %9.3f ms   (%.3f .. %.3f; %.0f GB/s)" % (m_ours + (nbytes / m_ours[0] / 1e6,)),
                  "  torch: %s" % how,
                  "                                    %9.3f ms   (%.3f .. %.3f; %.2f x map_fields; the results agree to %.1e)"
                  % (m_torch + (m_torch[0] / m_ours[0], agree)),
                  "  field_group_sums of the output    %9.3f ms   (%.3f .. %.3f; %.0f GB/s of its %.1f MB; map_fields takes %.2f x this)"
                  % (m_sums + (8 * N * L * q / m_sums[0] / 1e6, 8 * N * L * q / 1e6, m_ours[0] / m_sums[0]))]
        del values, mapped, ops
        torch.cuda.empty_cache()
    text = "\n".join(lines) + "\n"
    with open(out, "w") as f:
        f.write(text)
    print(text)


if __name__ == "__main__":
    main()

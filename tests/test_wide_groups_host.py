"""CPU tests of the wide-group limits: the header's BLUEST_MAX_GROUP, the entry points that report a plan's widest group and the
widest group phase 1's fused step accepts."""
import ctypes
import os
import re

from conftest import ROOT


def test_header_raises_the_group_limit_to_32():
    text = open(os.path.join(ROOT, "include", "bluest_hip.h")).read()
    m = re.search(r"#define\s+BLUEST_MAX_GROUP\s+(\d+)", text)
    assert m and int(m.group(1)) == 32
    assert int(re.search(r"#define\s+BLUEST_MAX_MODELS\s+(\d+)", text).group(1)) == 64


def test_library_exports_the_group_width_queries():
    from bluest_amd import _lib, build
    build.build()
    L = ctypes.CDLL(_lib.LIB_PATH)
    for name in ("bluest_plan_eval_ma_kmax", "bluest_plan_kmax", "bluest_group_pinv"):
        assert hasattr(L, name), name
        assert name in _lib.SIGNATURES
    assert _lib.SIGNATURES["bluest_plan_eval_ma_kmax"] == [ctypes.c_void_p, ctypes.POINTER(ctypes.c_int)]
    # no plan: an argument error, not a crash
    k = ctypes.c_int(-1)
    assert _lib.lib().bluest_plan_eval_ma_kmax(None, ctypes.byref(k)) == 1
    assert _lib.lib().bluest_plan_kmax(None, ctypes.byref(k)) == 1



def _cliques_loop(cp, K):
    """the per-clique enumeration: extend every (k-1)-clique c by each larger model linked to all of c"""
    import numpy as np
    nodes = cp.component
    out = [[(i,) for i in nodes]]
    for k in range(2, K + 1):
        out.append([c + (j,) for c in out[-1] for j in nodes if j > c[-1] and cp.linked[list(c)].all(axis=0)[j]])
    return [np.array(level, dtype=np.int64).reshape(-1, k + 1) for k, level in enumerate(out)]


def test_clique_enumeration_keeps_size_then_lexicographic_order():
    """the vectorised clique enumeration lists the same groups in the same order as the per-clique loop, on complete couplings,
    couplings with uncorrelated (0) and never-coupled (inf) pairs, a model outside model 0's component, and K beyond the size"""
    import numpy as np
    from itertools import combinations
    from bluest_amd.blue_models import _Coupling
    rng = np.random.RandomState(1)
    for t in range(40):
        M = int(rng.randint(1, 13))
        C = np.eye(M) + 0.5
        for _ in range(int(rng.randint(0, 2 * M))):
            a, b = rng.randint(M, size=2)
            if a != b:
                C[a, b] = C[b, a] = (0.0, np.inf)[rng.randint(2)]
        cp = _Coupling(C, True)
        for K in (1, 2, M, M + 2):
            got, want = cp.cliques(K), _cliques_loop(cp, K)
            assert len(got) == len(want) == K
            for a, b in zip(got, want):
                assert a.dtype == np.int64 and a.shape == b.shape and (a == b).all(), (t, K)
    cp = _Coupling(np.eye(12) + 0.5, True)
    for k, lv in enumerate(cp.cliques(12), start=1):
        assert (lv == np.array(list(combinations(range(12), k)), dtype=np.int64).reshape(-1, k)).all()

"""
One evaluation m -> (Phi(m), V(m), grad V(m), status) restated in 80-bit extended precision (np.longdouble), as the reference
defines it (bluest/misc.py:453-505):
    Phi      = sum_i m_i P_i^T B_i P_i                                  (misc.py:459-461)
    V        = (Phi[idx, idx] + delta I)^-1 [first, first]              idx = models of groups with |m_i| > 1e-6 (misc.py:463-477, :490)
    y        = row 0 of (Phi + delta I)^-1 on the support of Phi        (misc.py:487: pinv of the padded matrix = padded inverse)
    grad_i   = -y_g^T B_i y_g                                           (misc.py:493, cmisc.cpp:58-72)
B_i is given: the plan's own float64 group inverses for stored plans (so that only the evaluation kernels are measured), or the
longdouble inverse of C[g, g] (blocks_from_cov) for matrix-free plans.  No pseudo-inverse here: the restricted systems must be
regular (status SINGULAR is judged against the float64 OracleSAP instead).  numpy only.
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)          # unit roundoff of the evaluation under test is EPS / 2
EVAL_OK, EVAL_INF, EVAL_NO_MODEL0 = 0, 1, 2


def inv_ld(A):
    """batched Gauss-Jordan inverse in longdouble, no pivoting (SPD blocks): (G, k, k) -> (G, k, k)"""
    A = np.array(A, dtype=LD)
    G, k, _ = A.shape
    I = np.broadcast_to(np.eye(k, dtype=LD), (G, k, k)).copy()
    for p in range(k):
        piv = A[:, p, p][:, None].copy()
        A[:, p, :] /= piv
        I[:, p, :] /= piv
        for r in range(k):
            if r != p:
                f = A[:, r, p][:, None].copy()
                A[:, r, :] -= f * A[:, p, :]
                I[:, r, :] -= f * I[:, p, :]
    return I


def solve_ld(A, b):
    """x = A^-1 b in longdouble by Gauss-Jordan with partial pivoting (A: n x n, b: n)"""
    A = np.array(A, dtype=LD)
    x = np.array(b, dtype=LD)
    n = A.shape[0]
    for p in range(n):
        q = p + int(np.argmax(np.abs(A[p:, p])))
        if q != p:
            A[[p, q]] = A[[q, p]]
            x[[p, q]] = x[[q, p]]
        piv = A[p, p]
        A[p, :] /= piv
        x[p] /= piv
        f = A[:, p].copy()
        f[p] = 0
        A -= f[:, None] * A[p, :][None, :]
        x -= f * x[p]
    return x


def blocks_from_flat(sizes, flat):
    """list over k = 1..K of (L_k, k, k) longdouble blocks from the reference layout (concat over k of L_k * k * k doubles)"""
    out, at = [], 0
    for k, Lk in enumerate(sizes, start=1):
        Lk = int(Lk)
        out.append(np.asarray(flat[at:at + Lk * k * k], dtype=np.float64).reshape(Lk, k, k).astype(LD))
        at += Lk * k * k
    return out


def blocks_from_cov(C, groups):
    """list over k of (L_k, k, k): C[g, g]^-1 in longdouble"""
    C = np.asarray(C, dtype=LD)
    out = []
    for k, g in enumerate(groups, start=1):
        g = np.asarray(g, dtype=np.int64).reshape(-1, k)
        out.append(inv_ld(C[g[:, :, None], g[:, None, :]]) if len(g) else np.zeros((0, k, k), dtype=LD))
    return out


def phi_ld(N, groups, blocks, m, absolute=False):
    """Phi(m) = sum_i m_i P_i^T B_i P_i (N x N longdouble); absolute=True: sum_i |m_i| |P_i^T B_i P_i| (the scale of the
    rounding error of any float64 summation of the same terms) and the number of terms per entry"""
    m = np.asarray(m)
    PHI = np.zeros((N, N), dtype=LD)
    cnt = np.zeros((N, N), dtype=np.int64)
    at = 0
    for k, (g, B) in enumerate(zip(groups, blocks), start=1):
        g = np.asarray(g, dtype=np.int64).reshape(-1, k)
        mk = np.asarray(m[at:at + len(g)]).astype(LD)
        at += len(g)
        live = mk != 0
        if not live.any():
            continue
        t = mk[live][:, None, None] * B[live]
        rows, cols = g[live][:, :, None], g[live][:, None, :]
        rows, cols = np.broadcast_to(rows, t.shape), np.broadcast_to(cols, t.shape)
        np.add.at(PHI, (rows, cols), np.abs(t) if absolute else t)
        np.add.at(cnt, (rows, cols), 1)
    return (PHI, cnt) if absolute else PHI


def evaluate(N, groups, blocks, m, delta=0.0):
    """dict(status, V, grad (float64, local order), phi (longdouble), cond (float64 2-norm condition of V's system), idx)"""
    m = np.asarray(m)
    L = len(m)
    if np.abs(m).max() < 0.05:                                            # misc.py:464,484
        return dict(status=EVAL_INF, V=np.inf, grad=np.full(L, np.inf), phi=None, cond=1.0, idx=None)
    t1, t2 = np.zeros(N, bool), np.zeros(N, bool)
    at = 0
    for k, g in enumerate(groups, start=1):
        g = np.asarray(g, dtype=np.int64).reshape(-1, k)
        mk = m[at:at + len(g)]
        at += len(g)
        t1[g[np.abs(mk) > 1.0e-6].ravel()] = True                      # misc.py:453-457
        t2[g[mk != 0].ravel()] = True
    PHI = phi_ld(N, groups, blocks, m)
    if not t1.any():
        return dict(status=EVAL_NO_MODEL0, V=np.nan, grad=np.zeros(L), phi=PHI, cond=1.0, idx=None)
    idx1 = np.flatnonzero(t1)
    A = PHI[np.ix_(idx1, idx1)] + LD(delta) * np.eye(len(idx1), dtype=LD)
    V = solve_ld(A, np.eye(len(idx1), 1, dtype=LD).ravel())[0]          # first row of the restricted matrix (misc.py:490)
    status = EVAL_OK if idx1[0] == 0 else EVAL_NO_MODEL0
    idx2 = np.arange(N) if delta != 0 else np.flatnonzero(t2)
    y = np.zeros(N, dtype=LD)
    if idx2[0] == 0:                                                      # row 0 of pinv(Phi) is zero off the support
        A2 = PHI[np.ix_(idx2, idx2)] + LD(delta) * np.eye(len(idx2), dtype=LD)
        y[idx2] = solve_ld(A2, np.eye(len(idx2), 1, dtype=LD).ravel())
    grad = []
    for k, (g, B) in enumerate(zip(groups, blocks), start=1):
        yg = y[np.asarray(g, dtype=np.int64).reshape(-1, k)]
        grad.append(-np.einsum("ij,ijl,il->i", yg, B, yg))
    cond = float(np.linalg.cond(A.astype(np.float64)))
    return dict(status=status, V=float(V), grad=np.concatenate(grad).astype(np.float64), phi=PHI, cond=cond, idx=idx1)

"""
The reference of the pseudo-inverse tests (test_pinv_ref.py on the CPU, test_gpu_group_pinv.py and test_gpu_record_pinv.py on the
GPU): a cyclic Jacobi eigen-decomposition in np.longdouble (80-bit on x86-64: eps 1.1e-19, exponents to 2^16383, so the blocks
scaled by 2^515 and 2^-540 need no care here) and the pseudo-inverse by the kernels' rule, plus record_pinv, a restatement of what
k_pinv_from_record documents (csrc/plan.hip) and of the reference's variance_GH on a rank-deficient Phi (bluest/misc.py:484-490).
"""
import numpy as np

LD = np.longdouble
EPS = float(np.finfo(np.float64).eps)
CUT = 1e-15                                  # eigenvalues with |lambda| <= CUT max|lambda| are dropped (numpy.linalg.pinv's rcond)
EVAL_OK, EVAL_INF, EVAL_NO_MODEL0 = 0, 1, 2
MAX_SWEEPS = 60


def symmetrise(a):
    """0.5 (a_ij + a_ji) in float64, exactly as the kernels form it on load"""
    a = np.asarray(a, dtype=np.float64)
    assert a.ndim == 2 and a.shape[0] == a.shape[1]
    return 0.5 * (a + a.T)


def jacobi_eigh(a):
    """(w, V) with sym(a) = V diag(w) V^T in longdouble, w in the order the sweeps leave them on the diagonal.

    Cyclic Jacobi in the round-robin order (n/2 disjoint rotations per step, n - 1 steps per sweep; an odd size is padded with a
    zero row and column that no rotation couples).  A rotation is skipped when a_pq is zero or |a_pq| <= 2^-70 ||A||_F, six
    binary digits below the format's eps; the sweeps end when one of them rotates nothing."""
    A0 = symmetrise(a).astype(LD)
    k = A0.shape[0]
    n = k + (k & 1)
    A = np.zeros((n, n), dtype=LD)
    A[:k, :k] = A0
    V = np.eye(n, dtype=LD)
    if n < 2:
        return A0.diagonal().copy(), np.eye(k, dtype=LD)
    tol = LD(2.0) ** -70 * np.sqrt((A * A).sum())
    h, one, two = n // 2, LD(1), LD(2)
    tid = np.arange(1, h)
    for _sweep in range(MAX_SWEEPS):
        rotated = False
        for r in range(n - 1):
            a1 = np.concatenate(([r], (r + tid) % (n - 1)))
            b1 = np.concatenate(([n - 1], (r - tid) % (n - 1)))
            p, q = np.minimum(a1, b1), np.maximum(a1, b1)
            apq = A[p, q]
            rot = np.abs(apq) > tol
            if not rot.any():
                continue
            rotated = True
            safe = np.where(rot, apq, one)
            tau = (A[q, q] - A[p, p]) / (two * safe)
            t = np.where(tau >= 0, one, -one) / (np.abs(tau) + np.sqrt(one + tau * tau))
            t = np.where(rot, t, LD(0))
            c = one / np.sqrt(one + t * t)
            s = t * c
            Ap, Aq = A[p, :].copy(), A[q, :].copy()          # rows: J^T A
            A[p, :] = c[:, None] * Ap - s[:, None] * Aq
            A[q, :] = s[:, None] * Ap + c[:, None] * Aq
            Ap, Aq = A[:, p].copy(), A[:, q].copy()          # columns: (J^T A) J
            A[:, p] = c * Ap - s * Aq
            A[:, q] = s * Ap + c * Aq
            A[p, q] = np.where(rot, LD(0), A[p, q])           # the annihilated pair is zero, not its rounding residue
            A[q, p] = A[p, q]
            Vp, Vq = V[:, p].copy(), V[:, q].copy()
            V[:, p] = c * Vp - s * Vq
            V[:, q] = s * Vp + c * Vq
        if not rotated:
            break
    else:
        raise RuntimeError("the longdouble Jacobi sweeps did not converge")
    return A.diagonal()[:k].copy(), V[:k, :k].copy()


def kept(w):
    """which eigenvalues the kernels' rule inverts: |lambda| > 1e-15 max|lambda| (negative ones included)"""
    aw = np.abs(w)
    return aw > LD(CUT) * (aw.max() if len(aw) else LD(0))


def pinv_ld(a):
    """(pinv of sym(a) in longdouble, eigenvalues, eigenvectors)"""
    w, V = jacobi_eigh(a)
    keep = kept(w)
    inv = np.zeros_like(w)
    inv[keep] = LD(1) / w[keep]
    return (V * inv) @ V.T, w, V


def cond_kept(w):
    """max|lambda| / min|lambda| over the kept eigenvalues (1 for a zero block)"""
    aw = np.abs(w)[kept(w)]
    return float(aw.max() / aw.min()) if len(aw) else 1.0


def margins(w):
    """(smallest kept, largest dropped) eigenvalue, both relative to max|lambda|: the admission figures of a case.  (inf, 0)
    where there is none."""
    aw = np.abs(w)
    m = aw.max() if len(aw) else LD(0)
    if m == 0:
        return np.inf, 0.0
    keep = kept(w)
    lo = float((aw[keep] / m).min()) if keep.any() else np.inf
    hi = float((aw[~keep] / m).max()) if (~keep).any() else 0.0
    return lo, hi


def fro_err(got, want):
    """norm(got - want) / norm(want), Frobenius, formed in longdouble (0 / 0 counts as 0)"""
    got, want = np.asarray(got, dtype=LD), np.asarray(want, dtype=LD)
    den = np.sqrt((want * want).sum())
    num = np.sqrt(((got - want) ** 2).sum())
    return float(num / den) if den > 0 else float(num)


def max_err(got, want):
    """max|got - want| / max|want|: the measure of V and of v (0 / 0 counts as 0)"""
    got, want = np.atleast_1d(np.asarray(got, dtype=LD)), np.atleast_1d(np.asarray(want, dtype=LD))
    den = np.abs(want).max()
    num = np.abs(got - want).max()
    return float(num / den) if den > 0 else float(num)


def record_len(N):
    return N * N + 2 * N + 1


def make_record(Phi, s1, s2, big):
    """one Phi record: N*N entries of Phi (row-major), the flags s1[N], s2[N] and big as 0.0 / 1.0"""
    Phi = np.asarray(Phi, dtype=np.float64)
    N = Phi.shape[0]
    return np.concatenate([Phi.reshape(-1), np.asarray(s1, dtype=np.float64).reshape(N), np.asarray(s2, dtype=np.float64).reshape(N),
                           [1.0 if big else 0.0]])


def record_pinv(rec, N, delta):
    """dict V, v (N,), status, and the eigenvalues of each pass (for the bound), of one record.

    big == 0: INF, V = +inf, v = 0.  No s1 model: NO_MODEL0, V = NaN, v = 0.  Otherwise V = pinv(Phi[s1, s1] + delta I)[t, t] with t
    the first s1 model (NO_MODEL0 if that is not model 0), and v = row 0 of the pseudo-inverse on mask2, zero elsewhere, where
    mask2 is every model if delta != 0 and s2 otherwise; v = 0 if model 0 is outside mask2.  Longdouble V and v."""
    rec = np.asarray(rec, dtype=np.float64)
    assert rec.shape == (record_len(N),)
    Phi = rec[:N * N].reshape(N, N)
    s1, s2 = rec[N * N:N * N + N] > 0.0, rec[N * N + N:N * N + 2 * N] > 0.0
    big = rec[N * N + 2 * N] > 0.0
    v = np.zeros(N, dtype=LD)
    if not big:
        return {"V": LD(np.inf), "v": v, "status": EVAL_INF, "w": []}
    if not s1.any():
        return {"V": LD(np.nan), "v": v, "status": EVAL_NO_MODEL0, "w": []}
    mask2 = np.ones(N, dtype=bool) if delta != 0.0 else s2

    def restricted(mask):
        idx = np.flatnonzero(mask)
        sub = symmetrise(Phi[np.ix_(idx, idx)]) + float(delta) * np.eye(len(idx))     # float64, as the kernel loads it
        return (idx,) + pinv_ld(sub)

    idx1, P1, w1, _ = restricted(s1)
    ws = [w1]
    V = P1[0, 0]                                     # t = idx1[0], the first row of the restricted matrix
    if mask2[0]:
        if np.array_equal(mask2, s1):
            idx2, P2 = idx1, P1
        else:
            idx2, P2, w2, _ = restricted(mask2)
            ws.append(w2)
        v[idx2] = P2[0, :]
    return {"V": V, "v": v, "status": EVAL_OK if s1[0] else EVAL_NO_MODEL0, "w": ws}

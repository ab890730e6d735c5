// jacobi.hpp -- the parallel-ordered cyclic Jacobi eigendecomposition in LDS, shared by covproj.hip (proj(): 256 threads, up to
// 64 x 64) and mirrors.hip (k_group_pinv_wide: one wavefront, 17..32 models).
//
// Round-robin pairing: Mp/2 disjoint rotations per step, Mp - 1 steps per sweep, sweeps until a whole sweep rotates nothing.  The
// 2 x 2 blocks of A <- J^T A J are updated together and the transpose written alongside, so A stays exactly symmetric and every
// annihilated entry exactly zero; the rotations are compiled without contraction, whichever file includes this one.  Accurate to
// ~eps ||A|| whatever the eigenvalue order.
#pragma once
#include "common.hpp"

constexpr int JACOBI_MAX_SWEEPS = 40;        // never reached; bounded so that a kernel always ends
constexpr double JACOBI_REL_TOL = 1e-18;     // a rotation is skipped when |a_pq| <= JACOBI_REL_TOL * ||A||_F

// The rotation tolerance from amax = max|a| and ssq = sum (a / amax)^2 (0 when amax is 0), reduced by the caller:
// ||A||_F = max|a| * sqrt(sum (a / max|a|)^2).  A plain sum of a^2 is inf from entries of 1.4e154 on, and an infinite tolerance
// would skip every rotation and report convergence.
__device__ __forceinline__ double jacobi_tol(double amax, double ssq) { return JACOBI_REL_TOL * amax * sqrt(ssq); }

// Eigendecomposition of the symmetric Mp x Mp matrix A (Mp even: an odd size is padded with a zero row and column, which are
// never coupled, so the pad's rotations are identities), row stride LD, by all NT threads of the workgroup.  On entry A, V = I and
// tol are visible to every thread; on return the diagonal of A holds the eigenvalues and the first `vrows` rows of V the
// eigenvectors (vrows = the unpadded size: the pad's row stays e_pad).  rc, rs, rt, rp, rq hold Mp/2 entries each.  Returns whether
// a sweep ended with no rotation, the same in every thread.  Mp <= 2 WAVE: the threads that choose the rotations are in thread 0's
// wavefront, whose LDS operations execute in order, so its reset of *rotated needs no barrier of its own.
template <int NT>
__device__ __forceinline__ bool jacobi_eigh_lds(double *A, double *V, int Mp, int vrows, int LD, double tol, double *rc, double *rs,
                                                double *rt, int *rp, int *rq, int *rotated)
{
#pragma clang fp contract(off)
    const int tid = threadIdx.x, h = Mp / 2;
    bool converged = false;
    for (int sweep = 0; sweep < JACOBI_MAX_SWEEPS && !converged; sweep++) {
        if (tid == 0) *rotated = 0;
        for (int r = 0; r < Mp - 1; r++) {
            if (tid < h) {                   // round-robin pairing: (r, Mp-1) and (r+k, r-k) mod (Mp-1)
                int a, b;
                if (tid == 0) { a = r; b = Mp - 1; }
                else          { a = (r + tid) % (Mp - 1); b = (r - tid + (Mp - 1)) % (Mp - 1); }
                const int p = min(a, b), q = max(a, b);
                const double apq = A[p * LD + q];
                double c = 1.0, s = 0.0, t = 0.0;
                if (fabs(apq) > tol) {       // Golub & Van Loan, sym.schur2
                    const double app = A[p * LD + p], aqq = A[q * LD + q];
                    const double tau = (aqq - app) / (2.0 * apq);
                    if (fabs(tau) > 1e150) t = 0.5 / tau;
                    else t = (tau >= 0.0 ? 1.0 : -1.0) / (fabs(tau) + sqrt(1.0 + tau * tau));
                    c = 1.0 / sqrt(1.0 + t * t);
                    s = t * c;
                    *rotated = 1;
                }
                rp[tid] = p; rq[tid] = q; rc[tid] = c; rs[tid] = s; rt[tid] = t;
            }
            __syncthreads();
            // A <- J^T A J on the 2x2 blocks (P <= Q, the transpose written too: A stays exactly symmetric)
            const int nblk = h * (h + 1) / 2;
            for (int b = tid; b < nblk; b += NT) {
                int Pb = 0, rem = b;
                while (rem >= h - Pb) { rem -= h - Pb; Pb++; }
                const int Qb = Pb + rem;
                const int p1 = rp[Pb], q1 = rq[Pb], p2 = rp[Qb], q2 = rq[Qb];
                const double c1 = rc[Pb], s1 = rs[Pb], c2 = rc[Qb], s2 = rs[Qb];
                if (Pb == Qb) {
                    if (s1 != 0.0) {
                        const double t1 = rt[Pb], apq = A[p1 * LD + q1];
                        A[p1 * LD + p1] = A[p1 * LD + p1] - t1 * apq;
                        A[q1 * LD + q1] = A[q1 * LD + q1] + t1 * apq;
                        A[p1 * LD + q1] = 0.0;
                        A[q1 * LD + p1] = 0.0;
                    }
                    continue;
                }
                if (s1 == 0.0 && s2 == 0.0) continue;
                const double b11 = A[p1 * LD + p2], b12 = A[p1 * LD + q2];
                const double b21 = A[q1 * LD + p2], b22 = A[q1 * LD + q2];
                const double r11 = c1 * b11 - s1 * b21, r12 = c1 * b12 - s1 * b22;     // rows: J_P^T B
                const double r21 = s1 * b11 + c1 * b21, r22 = s1 * b12 + c1 * b22;
                const double n11 = c2 * r11 - s2 * r12, n12 = s2 * r11 + c2 * r12;     // columns: (J_P^T B) J_Q
                const double n21 = c2 * r21 - s2 * r22, n22 = s2 * r21 + c2 * r22;
                A[p1 * LD + p2] = n11; A[p1 * LD + q2] = n12; A[q1 * LD + p2] = n21; A[q1 * LD + q2] = n22;
                A[p2 * LD + p1] = n11; A[q2 * LD + p1] = n12; A[p2 * LD + q1] = n21; A[q2 * LD + q1] = n22;
            }
            // V <- V J
            for (int it = tid; it < vrows * h; it += NT) {
                const int i = it / h, Q = it % h;
                const double s = rs[Q];
                if (s == 0.0) continue;
                const double c = rc[Q];
                const int p = rp[Q], q = rq[Q];
                const double vp = V[i * LD + p], vq = V[i * LD + q];
                V[i * LD + p] = c * vp - s * vq;
                V[i * LD + q] = s * vp + c * vq;
            }
            __syncthreads();
        }
        converged = *rotated == 0;           // read by every thread after the step's barrier
        __syncthreads();                     // before thread 0 resets the flag
    }
    return converged;
}

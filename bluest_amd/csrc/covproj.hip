// covproj.hip -- Part 8 of include/bluest_hip.h: the projection of a (partially known) covariance onto the SPD matrices
// (bluest/blue_models.py:348-433 with the SPG solver of bluest/spg.py:1-132).
//
// One workgroup per output, one launch for all outputs; the whole SPG loop runs inside the workgroup.  A projection
//   proj(X) = V max(l, thr) V^T,   (l, V) = eigh((X + X^T) / 2)
// is a parallel-ordered cyclic Jacobi eigendecomposition in LDS (jacobi.hpp; round-robin pairing: M/2 disjoint rotations per step,
// M-1 steps per sweep, sweeps until a whole sweep rotates nothing), accurate to ~eps ||X|| whatever the eigenvalue order.  The
// matrix and its eigenvectors (two 64 x 65 float64 arrays, 65 KB) live in LDS; the SPG vectors (x, g, d, trial point, ...) in
// the workgroup's own slice of global scratch.
//
// The branches that decide the trajectory (nonmonotone Armijo acceptance, safeguarded interpolation, the sdoty <= 0 case, the
// stopping test) follow the reference expression by expression (float64, no contraction).
#include "jacobi.hpp"

#pragma clang fp contract(off)

namespace {

constexpr int BLK = 256;
constexpr int NWAVE = BLK / WAVE;
constexpr int MAXM = BLUEST_MAX_MODELS;
constexpr int LD = MAXM + 1;                 // LDS row stride (doubles)
constexpr int HALF = MAXM / 2;
constexpr int NVEC = 8;                      // global scratch vectors per output

struct Params {
    int M, hlen;
    double thr, eps, lmin, lmax;
    long long maxit, max_fevals;
};

struct Lds {
    double A[MAXM * LD];
    double V[MAXM * LD];
    double rc[HALF], rs[HALF], rt[HALF];
    int rp[HALF], rq[HALF];
    double red[NWAVE];
    double hist[BLUEST_COVPROJ_MAX_HISTORY];
    int rotated;
};

__device__ __forceinline__ double block_sum(double v, double *red)
{   // the same value in every thread; fixed order: butterfly within each wave, then waves 0..NWAVE-1
    v = wave_sum(v);
    const int w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) red[w] = v;
    __syncthreads();
    double r = 0.0;
#pragma unroll
    for (int i = 0; i < NWAVE; i++) r += red[i];
    __syncthreads();
    return r;
}

__device__ __forceinline__ double block_max(double v, double *red)
{
    v = wave_max(v);
    const int w = threadIdx.x / WAVE;
    if ((threadIdx.x & (WAVE - 1)) == 0) red[w] = v;
    __syncthreads();
    double r = red[0];
#pragma unroll
    for (int i = 1; i < NWAVE; i++) r = fmax(r, red[i]);
    __syncthreads();
    return r;
}

// out = proj(in): symmetric part of `in` (or, with lower_only, the matrix given by its lower triangle, as LAPACK's eigh reads
// it), eigenvalues clipped at thr, reassembled.  `in` and `out` are M x M row-major in global memory and may alias.  Returns
// false when the Jacobi sweeps did not converge (never seen; bounded so that the kernel always ends).
__device__ bool proj(const Params &P, const double *in, double *out, Lds &L, bool lower_only)
{
    const int M = P.M, N = M * M, tid = threadIdx.x;
    const int Mp = M + (M & 1);              // padded to even: the pad index is never coupled, its rotations are identities
    __syncthreads();                         // `in` was written by other threads
    double amax = 0.0;
    for (int idx = tid; idx < Mp * Mp; idx += BLK) {
        const int i = idx / Mp, j = idx % Mp;
        double a = 0.0;
        if (i < M && j < M) {
            if (lower_only) a = i >= j ? in[i * M + j] : in[j * M + i];
            else            a = (in[i * M + j] + in[j * M + i]) / 2;
        }
        L.A[i * LD + j] = a;
        L.V[i * LD + j] = (i == j) ? 1.0 : 0.0;
        amax = fmax(amax, fabs(a));
    }
    amax = block_max(amax, L.red);           // its barriers also publish A and V
    double nrm = 0.0;                        // sum (a / max|a|)^2: see jacobi_tol
    if (amax > 0.0)
        for (int idx = tid; idx < Mp * Mp; idx += BLK) {
            const double a = L.A[(idx / Mp) * LD + idx % Mp] / amax;
            nrm += a * a;
        }
    nrm = block_sum(nrm, L.red);
    const bool converged = jacobi_eigh_lds<BLK>(L.A, L.V, Mp, M, LD, jacobi_tol(amax, nrm), L.rc, L.rs, L.rt, L.rp, L.rq, &L.rotated);
    // clip on the diagonal (l[l < eps] = eps), then out = V diag(l) V^T, upper triangle computed and mirrored
    for (int k = tid; k < M; k += BLK) {
        const double l = L.A[k * LD + k];
        L.A[k * LD + k] = (l < P.thr) ? P.thr : l;
    }
    __syncthreads();
    for (int idx = tid; idx < N; idx += BLK) {
        const int i = idx / M, j = idx % M;
        if (j < i) continue;
        double acc = 0.0;
        for (int k = 0; k < M; k++) acc += (L.V[i * LD + k] * L.A[k * LD + k]) * L.V[j * LD + k];
        out[i * M + j] = acc;
        out[j * M + i] = acc;
    }
    __syncthreads();
    return converged;
}

// am(v, mask**2) of the reference: zero where |w| < 1e-15, v * w elsewhere
__device__ __forceinline__ double am(double v, double w) { return fabs(w) < 1.0e-15 ? 0.0 : v * w; }

__global__ void __launch_bounds__(BLK) k_covproj(Params P, const double *__restrict__ Cg, const double *__restrict__ maskg,
                                                 double *__restrict__ scratch, double *__restrict__ Xout, double *__restrict__ fout,
                                                 double *__restrict__ gpout, long long *__restrict__ itout,
                                                 long long *__restrict__ cntout, int32_t *__restrict__ info)
{
    __shared__ Lds L;
    const int o = blockIdx.x, tid = threadIdx.x;
    const int M = P.M, N = M * M;
    const double *C = Cg + (size_t)o * N;
    const double *mask = maskg + (size_t)o * N;
    double *ws = scratch + (size_t)o * NVEC * N;
    double *Cm = ws, *W = ws + N, *x = ws + 2 * N, *g = ws + 3 * N, *d = ws + 4 * N, *xn = ws + 5 * N, *gn = ws + 6 * N,
           *t = ws + 7 * N;
    double *X = Xout + (size_t)o * N;

    // inputs: W = mask**2, Cm = C with the unmasked entries zeroed (NaN there is "not coupled")
    double bad = 0.0, unknown = 0.0;
    for (int i = tid; i < N; i += BLK) {
        const double m = mask[i], c = C[i];
        W[i] = m * m;
        const bool used = !(fabs(m) < 1.0e-14);
        Cm[i] = used ? c : 0.0;
        if (!isfinite(m) || (used && !isfinite(c))) bad = 1.0;
        if (!used) unknown = 1.0;
    }
    bad = block_max(bad, L.red);
    unknown = block_max(unknown, L.red);
    auto finish = [&](double f, double gpmax, long long it, long long count, int status) {
        if (tid == 0) { fout[o] = f; gpout[o] = gpmax; itout[o] = it; cntout[o] = count; info[o] = status; }
    };
    if (bad != 0.0) {
        for (int i = tid; i < N; i += BLK) X[i] = C[i];
        finish(NAN, NAN, 0, 0, BLUEST_COVPROJ_NONFINITE);
        return;
    }

    if (unknown == 0.0) {
        // every entry known: one clip of eigh(C) (which reads the lower triangle), err = ||C - C_new||_F
        if (!proj(P, C, X, L, true)) { finish(NAN, NAN, 0, 0, BLUEST_COVPROJ_NOEIG); return; }
        double e = 0.0;
        for (int i = tid; i < N; i += BLK) { const double r = C[i] - X[i]; e += r * r; }
        e = sqrt(block_sum(e, L.red));
        finish(e, 0.0, 0, 0, BLUEST_COVPROJ_OK);
        return;
    }

    auto feval = [&](const double *v) -> double {            // 0.5 * sum(am(v - C, mask**2)**2)
        double s = 0.0;
        for (int i = tid; i < N; i += BLK) { const double r = am(v[i] - Cm[i], W[i]); s += r * r; }
        return 0.5 * block_sum(s, L.red);
    };
    bool eig_ok = true;
    // x0 = proj(am(C, |mask| > 1e-14)); spg() then projects it once more
    eig_ok &= proj(P, Cm, x, L, false);
    eig_ok &= proj(P, x, x, L, false);
    double f = feval(x);
    for (int i = tid; i < N; i += BLK) { g[i] = am(x[i] - Cm[i], W[i]); t[i] = x[i] - g[i]; }
    long long it = 0, count = 1;
    for (int k = tid; k < P.hlen; k += BLK) L.hist[k] = (k == 0) ? f : -INFINITY;
    eig_ok &= proj(P, t, t, L, false);
    double gpmax = 0.0;
    for (int i = tid; i < N; i += BLK) gpmax = fmax(gpmax, fabs(t[i] - x[i]));
    gpmax = block_max(gpmax, L.red);
    double lmbda = (gpmax > 1.0e-15) ? fmin(P.lmax, fmax(P.lmin, 1.0 / gpmax)) : 0.0;

    while (gpmax > P.eps && it < P.maxit && count < P.max_fevals) {
        if (!eig_ok) break;
        it += 1;
        // d = proj(x - lmbda g) - x
        for (int i = tid; i < N; i += BLK) d[i] = x[i] - lmbda * g[i];
        eig_ok &= proj(P, d, d, L, false);
        double gd = 0.0;
        for (int i = tid; i < N; i += BLK) { d[i] = d[i] - x[i]; gd += g[i] * d[i]; }
        gd = block_sum(gd, L.red);
        // nonmonotone line search (bluest/spg.py:3-35)
        double fmx = L.hist[0];
        for (int k = 1; k < P.hlen; k++) fmx = fmax(fmx, L.hist[k]);
        const double gamma = 1.0e-4, sigma_min = 0.1, sigma_max = 0.9;
        double alpha = 1.0;
        for (int i = tid; i < N; i += BLK) xn[i] = x[i] + alpha * d[i];
        double fnew = feval(xn);
        count += 1;
        while (fnew > fmx + gamma * alpha * gd && count < P.max_fevals) {
            if (alpha <= sigma_min) {
                alpha *= 0.5;
            } else {
                double alpha_t = -0.5 * (alpha * alpha) * gd / (fnew - f - alpha * gd);
                if (alpha_t < sigma_min || alpha_t > sigma_max * alpha) alpha_t = 0.5 * alpha;
                alpha = alpha_t;
            }
            for (int i = tid; i < N; i += BLK) xn[i] = x[i] + alpha * d[i];
            fnew = feval(xn);
            count += 1;
        }
        if (!(fnew <= fmx + gamma * alpha * gd)) {           // linesearch_info == 2: x stays the last accepted point
            for (int i = tid; i < N; i += BLK) X[i] = x[i];
            finish(f, gpmax, it, count, BLUEST_COVPROJ_MAXFEV);
            return;
        }
        f = fnew;
        __syncthreads();                                     // every thread has read the history
        if (tid == 0) L.hist[it % P.hlen] = f;
        double sdots = 0.0, sdoty = 0.0;
        for (int i = tid; i < N; i += BLK) {
            const double gni = am(xn[i] - Cm[i], W[i]);
            const double si = xn[i] - x[i], yi = gni - g[i];
            sdots += si * si;
            sdoty += si * yi;
            x[i] = xn[i];
            g[i] = gni;
            t[i] = x[i] - g[i];
        }
        sdots = block_sum(sdots, L.red);
        sdoty = block_sum(sdoty, L.red);
        eig_ok &= proj(P, t, t, L, false);
        gpmax = 0.0;
        for (int i = tid; i < N; i += BLK) gpmax = fmax(gpmax, fabs(t[i] - x[i]));
        gpmax = block_max(gpmax, L.red);
        if (sdoty <= 0) lmbda = P.lmax;
        else lmbda = fmin(P.lmax, fmax(P.lmin, sdots / sdoty));
    }
    for (int i = tid; i < N; i += BLK) X[i] = x[i];
    int status;
    if (!eig_ok) status = BLUEST_COVPROJ_NOEIG;
    else if (gpmax <= P.eps) status = BLUEST_COVPROJ_OK;
    else if (it >= P.maxit) status = BLUEST_COVPROJ_MAXIT;
    else status = BLUEST_COVPROJ_MAXFEV;
    finish(f, gpmax, it, count, status);
}

}  // namespace

extern "C" int bluest_cov_project(int M, int n_out, const double *C, const double *mask, double spd_threshold, double eps,
                                  double lmbda_min, double lmbda_max, int64_t maxit, int64_t max_fevals, int hlength,
                                  double *X_out, double *f_out, double *gpmax_out, int64_t *it_out, int64_t *count_out,
                                  int32_t *info_out, void *stream)
{
    if (M < 1 || M > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "M=%d out of range (1..%d)", M, BLUEST_MAX_MODELS);
    if (n_out < 1 || n_out > BLUEST_COVPROJ_MAX_OUTPUTS)
        return fail(BLUEST_ERR_ARG, "n_out=%d out of range (1..%d)", n_out, BLUEST_COVPROJ_MAX_OUTPUTS);
    if (hlength < 1 || hlength > BLUEST_COVPROJ_MAX_HISTORY)
        return fail(BLUEST_ERR_ARG, "hlength=%d out of range (1..%d)", hlength, BLUEST_COVPROJ_MAX_HISTORY);
    if (!C || !mask || !X_out || !f_out || !gpmax_out || !it_out || !count_out || !info_out) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!std::isfinite(spd_threshold) || !std::isfinite(eps) || std::isnan(lmbda_min) || std::isnan(lmbda_max) || maxit < 0 ||
        max_fevals < 0)
        return fail(BLUEST_ERR_ARG, "spd_threshold, eps, lmbda_min, lmbda_max, maxit or max_fevals out of range");
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const size_t N = (size_t)M * M, mat = (size_t)n_out * N * 8;
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_c = take(mat), o_m = take(mat), o_x = take(mat), o_ws = take(mat * NVEC);
    const size_t o_f = take(n_out * 8), o_g = take(n_out * 8), o_it = take(n_out * 8), o_cn = take(n_out * 8), o_in = take(n_out * 4);
    char *dv = nullptr;
    HIP_TRY(hipMalloc(&dv, off));
    struct Free { char *p; ~Free() { if (p) (void)hipFree(p); } } guard{dv};
    HIP_TRY(hipMemcpyAsync(dv + o_c, C, mat, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_m, mask, mat, hipMemcpyHostToDevice, st));
    Params P;
    P.M = M; P.hlen = hlength; P.thr = spd_threshold; P.eps = eps; P.lmin = lmbda_min; P.lmax = lmbda_max;
    P.maxit = maxit; P.max_fevals = max_fevals;
    hipLaunchKernelGGL(k_covproj, dim3(n_out), dim3(BLK), 0, st, P, (const double *)(dv + o_c), (const double *)(dv + o_m),
                       (double *)(dv + o_ws), (double *)(dv + o_x), (double *)(dv + o_f), (double *)(dv + o_g),
                       (long long *)(dv + o_it), (long long *)(dv + o_cn), (int32_t *)(dv + o_in));
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(X_out, dv + o_x, mat, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(f_out, dv + o_f, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(gpmax_out, dv + o_g, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(it_out, dv + o_it, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(count_out, dv + o_cn, n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(info_out, dv + o_in, n_out * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

// pilot.hip -- Part 10 of include/bluest_hip.h: the sums over pilot samples that the covariance and MLMC-variance estimates are
// made of (bluest/blue_models.py:326-346, accumulated by bluest/blue_fn.py:147-167 one Python call per pair and sample).
//
// Two launches, no atomics, nothing sized by the device: the result is a function of the input and of BLUEST_PILOT_CHUNK only.
//   k_pilot_partial  grid (chunk, output): stages BLUEST_PILOT_CHUNK samples x L models in LDS as they lie in memory (row = one
//                    sample), then every thread walks the samples in ascending order with its pairs' sums in f64 registers.
//   k_pilot_fold     grid (pair block, output): adds the chunks in ascending order, writes the outputs, mirrors sumsc.
//
// The pair -> thread map (wrapped diagonals, conflict-free LDS reads) is in staging.hpp.
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
constexpr int CHUNK = BLUEST_PILOT_CHUNK;
constexpr int KMAX = (BLUEST_MAX_MODELS * (BLUEST_MAX_MODELS + 1) / 2 + BLK - 1) / BLK;     // pairs per thread: 9
static_assert((size_t)CHUNK * BLUEST_MAX_MODELS * sizeof(double) <= 64 * 1024, "the staged chunk must fit the default LDS limit");

// part: [output][chunk][slot][pair], slot 0 = sum y_lo y_hi, and with DIFF 1 = sum (y_lo - y_hi), 2 = sum (y_lo - y_hi)^2;
// parte: [output][chunk][L] = sum y_i
template <bool DIFF>
__global__ __launch_bounds__(BLK) void k_pilot_partial(int64_t N, int L, const double *__restrict__ values, double *__restrict__ part,
                                                       double *__restrict__ parte)
{
    extern __shared__ double tile[];
    constexpr int NS = DIFF ? 3 : 1;
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x, o = blockIdx.y, nchunks = gridDim.x;
    const int64_t s0 = c * CHUNK;
    const int ns = (int)min((int64_t)CHUNK, N - s0);
    const double *src = values + (o * N + s0) * L;
    const int cnt = ns * L;
    for (int t = tid; t < cnt; t += BLK) tile[t] = src[t];
    __syncthreads();

    const int npairs = n_pairs(L), kcount = (npairs + BLK - 1) / BLK;
    int lo[KMAX], hi[KMAX];
    double p[KMAX], r[KMAX], w[KMAX];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int q = tid + k * BLK;
        lo[k] = hi[k] = 0;
        if (q < npairs) pair_of(q, L, lo[k], hi[k]);
        p[k] = r[k] = w[k] = 0.0;
    }
    const int ecol = tid < L ? tid : 0;
    double e = 0.0;
    for (int s = 0; s < ns; s++) {
        const double *row = tile + s * L;
        e += row[ecol];
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            if (k < kcount) {
                const double a = row[lo[k]], b = row[hi[k]];
                p[k] = fma(a, b, p[k]);
                if (DIFF) {
                    const double d = a - b;
                    r[k] += d;
                    w[k] = fma(d, d, w[k]);
                }
            }
        }
    }
    double *dst = part + (o * nchunks + c) * NS * (int64_t)npairs;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int q = tid + k * BLK;
        if (q < npairs) {
            dst[q] = p[k];
            if (DIFF) {
                dst[npairs + q] = r[k];
                dst[2 * npairs + q] = w[k];
            }
        }
    }
    if (tid < L) parte[(o * nchunks + c) * L + tid] = e;
}

template <bool DIFF>
__global__ __launch_bounds__(BLK) void k_pilot_fold(int64_t nchunks, int L, const double *__restrict__ part,
                                                    const double *__restrict__ parte, double *__restrict__ sumse,
                                                    double *__restrict__ sumsc, double *__restrict__ sumsd1, double *__restrict__ sumsd2)
{
    constexpr int NS = DIFF ? 3 : 1;
    const int npairs = n_pairs(L);
    const int q = blockIdx.x * BLK + threadIdx.x;
    const int64_t o = blockIdx.y;
    if (q >= npairs) return;
    const double *src = part + o * nchunks * NS * (int64_t)npairs + q;
    const int64_t step = (int64_t)NS * npairs;
    double p = 0.0, r = 0.0, w = 0.0;
    for (int64_t c = 0; c < nchunks; c++) {
        p += src[c * step];
        if (DIFF) {
            r += src[c * step + npairs];
            w += src[c * step + 2 * npairs];
        }
    }
    int lo, hi;
    pair_of(q, L, lo, hi);
    const int64_t mat = o * L * L;
    sumsc[mat + lo * L + hi] = p;
    sumsc[mat + hi * L + lo] = p;
    if (DIFF && lo < hi) {                                  // the other entries were set to zero before the launch
        sumsd1[mat + lo * L + hi] = r;
        sumsd2[mat + lo * L + hi] = w;
    }
    if (q < L) {                                            // the first diagonal has L pairs: npairs >= L
        double e = 0.0;
        for (int64_t c = 0; c < nchunks; c++) e += parte[(o * nchunks + c) * L + q];
        sumse[o * L + q] = e;
    }
}

}  // namespace

extern "C" int bluest_pilot_stats(int64_t N, int L, int n_out, const double *values, double *sumse, double *sumsc, double *sumsd1,
                                  double *sumsd2, void *stream)
{
    if (L < 1 || L > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "L=%d out of range (1..%d)", L, BLUEST_MAX_MODELS);
    if (n_out < 1 || n_out > BLUEST_PILOT_MAX_OUTPUTS)
        return fail(BLUEST_ERR_ARG, "n_out=%d out of range (1..%d)", n_out, BLUEST_PILOT_MAX_OUTPUTS);
    if (N < 1) return fail(BLUEST_ERR_ARG, "N=%lld: at least one sample is needed", (long long)N);
    const int64_t nchunks = (N - 1) / CHUNK + 1;
    if (nchunks > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "N=%lld: more than 2^31 - 1 chunks of %d samples", (long long)N, CHUNK);
    if (!values || !sumse || !sumsc) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((sumsd1 == nullptr) != (sumsd2 == nullptr)) return fail(BLUEST_ERR_ARG, "sumsd1 and sumsd2 must both be given or both be null");
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool diff = sumsd1 != nullptr, staged = !on_device(values);
    const int npairs = n_pairs(L), ns = diff ? 3 : 1;
    const size_t in_bytes = (size_t)n_out * (size_t)N * L * 8, mat = (size_t)n_out * L * L * 8, vec = (size_t)n_out * L * 8;
    DeviceArena arena;
    const size_t o_in = arena.take(staged ? in_bytes : 0), o_part = arena.take((size_t)n_out * nchunks * ns * npairs * 8),
                 o_pe = arena.take((size_t)n_out * nchunks * L * 8), o_se = arena.take(vec), o_sc = arena.take(mat),
                 o_d1 = arena.take(diff ? mat : 0), o_d2 = arena.take(diff ? mat : 0);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_in = values;
    if (staged) {
        HIP_TRY(hipMemcpyAsync(dv + o_in, values, in_bytes, hipMemcpyHostToDevice, st));
        d_in = (const double *)(dv + o_in);
    }
    double *d_part = (double *)(dv + o_part), *d_pe = (double *)(dv + o_pe), *d_se = (double *)(dv + o_se), *d_sc = (double *)(dv + o_sc);
    double *d_d1 = diff ? (double *)(dv + o_d1) : nullptr, *d_d2 = diff ? (double *)(dv + o_d2) : nullptr;
    const dim3 g1((unsigned)nchunks, (unsigned)n_out), g2((unsigned)((npairs + BLK - 1) / BLK), (unsigned)n_out);
    const size_t lds = (size_t)CHUNK * L * 8;
    if (diff) {
        HIP_TRY(hipMemsetAsync(d_d1, 0, mat, st));
        HIP_TRY(hipMemsetAsync(d_d2, 0, mat, st));
        hipLaunchKernelGGL(k_pilot_partial<true>, g1, dim3(BLK), lds, st, N, L, d_in, d_part, d_pe);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pilot_fold<true>, g2, dim3(BLK), 0, st, nchunks, L, (const double *)d_part, (const double *)d_pe, d_se,
                           d_sc, d_d1, d_d2);
    } else {
        hipLaunchKernelGGL(k_pilot_partial<false>, g1, dim3(BLK), lds, st, N, L, d_in, d_part, d_pe);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_pilot_fold<false>, g2, dim3(BLK), 0, st, nchunks, L, (const double *)d_part, (const double *)d_pe, d_se,
                           d_sc, d_d1, d_d2);
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sumse, d_se, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sumsc, d_sc, mat, hipMemcpyDeviceToHost, st));
    if (diff) {
        HIP_TRY(hipMemcpyAsync(sumsd1, d_d1, mat, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(sumsd2, d_d2, mat, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

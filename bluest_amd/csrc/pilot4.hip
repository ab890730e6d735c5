// pilot4.hip -- Part 14 of include/bluest_hip.h: the sums over pilot samples, up to the fourth order, that the standard errors of
// the covariance and MLMC-variance estimates are made of (bluest_amd/pilot_errors.py).  One more pass over the array Part 10 reads.
//
// Same contract as pilot.hip: no atomics, nothing sized by the device, every operation in a fixed order, so the result is a
// function of the values, the shift and BLUEST_PILOT_CHUNK only.  Two launches:
//   k_p4_partial<DIFFS>  grid (chunk, output): stages BLUEST_PILOT_CHUNK samples x L models in LDS, then every thread walks the
//                        samples in ascending order with the sums of its pairs in f64 registers.
//        <false>         the pair sums alone (tpow null): d_lo d_hi, d_lo^2 d_hi, d_lo d_hi^2, d_lo^2 d_hi^2.  The chunk is staged
//                        MINUS THE SHIFT (the 128 x 64 chunk fills the default 64 KB, so the shift has no room in LDS).
//        <true>          also t, t^2, t^3, t^4 of t = (y_lo - y_hi) - (a_lo - a_hi) from the SAME two LDS reads per pair and sample:
//                        t needs the values as they lie, so the chunk is staged raw and a_lo, a_hi stay in registers.  At L = 64
//                        that is nine pairs x eight accumulators per thread: 240 VGPRs, no scratch, and the two waves per SIMD
//                        that 64 KB of LDS per workgroup allow anyway (DESIGN.md section 14 has the compiler's figures and the
//                        measurement against two separate passes).
//   k_p4_fold            grid (block of (slot, pair), output): adds the chunks in ascending order and writes the outputs.
// The pair -> thread map is staging.hpp's.
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
constexpr int CHUNK = BLUEST_PILOT_CHUNK;
constexpr int KMAX = (BLUEST_MAX_MODELS * (BLUEST_MAX_MODELS + 1) / 2 + BLK - 1) / BLK;     // pairs per thread: 9
constexpr int NS = 4;                                                                       // pair sums per pair; as many difference sums
static_assert((size_t)CHUNK * BLUEST_MAX_MODELS * sizeof(double) <= 64 * 1024, "the staged chunk must fit the default LDS limit");

// shift: a_i of output o at shift[o * shift_stride + i] (the first sample of `values`, or the caller's array)
// part:  [output][chunk][slot][pair], slot 0 = S11, 1 = S21[lo][hi], 2 = S21[hi][lo], 3 = S22, and with DIFFS slot 3 + k = sum t^k;
// parte: [output][chunk][L] = sum d_i
// DIFFS false: the chunk is staged minus the shift.  DIFFS true: t needs the values as they lie, so the chunk is staged raw and a
// thread keeps a_lo and a_hi of its pairs in registers; d = y - a is the same single rounding in either place.
template <bool DIFFS>
__global__ __launch_bounds__(BLK) void k_p4_partial(int64_t N, int L, const double *__restrict__ values, const double *__restrict__ shift,
                                                    int64_t shift_stride, double *__restrict__ part, double *__restrict__ parte)
{
    extern __shared__ double tile[];
    constexpr int NSL = DIFFS ? 2 * NS : NS;
    const int tid = threadIdx.x;
    const int64_t c = blockIdx.x, o = blockIdx.y, nchunks = gridDim.x;
    const int64_t s0 = c * CHUNK;
    const int ns = (int)min((int64_t)CHUNK, N - s0);
    const double *src = values + (o * N + s0) * L;
    const double *sh = shift + o * shift_stride;
    const int cnt = ns * L;
    for (int t = tid; t < cnt; t += BLK) tile[t] = DIFFS ? src[t] : src[t] - sh[t % L];   // d = y - a: one rounding
    __syncthreads();

    const int npairs = n_pairs(L), kcount = (npairs + BLK - 1) / BLK;
    int lo[KMAX], hi[KMAX];
    double alo[DIFFS ? KMAX : 1], ahi[DIFFS ? KMAX : 1];
    double acc[KMAX][NSL];
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int q = tid + k * BLK;
        lo[k] = hi[k] = 0;
        if (q < npairs) pair_of(q, L, lo[k], hi[k]);
        if constexpr (DIFFS) { alo[k] = sh[lo[k]]; ahi[k] = sh[hi[k]]; }
#pragma unroll
        for (int j = 0; j < NSL; j++) acc[k][j] = 0.0;
    }
    const int ecol = tid < L ? tid : 0;
    const double ea = DIFFS ? sh[ecol] : 0.0;
    double e = 0.0;
    for (int s = 0; s < ns; s++) {
        const double *row = tile + s * L;
        e += DIFFS ? row[ecol] - ea : row[ecol];
#pragma unroll
        for (int k = 0; k < KMAX; k++) {
            if (k < kcount) {
                double a = row[lo[k]], b = row[hi[k]];
                if constexpr (DIFFS) {
                    const double t = (a - b) - (alo[k] - ahi[k]);       // each inner difference rounded once, then the outer one
                    const double q = __dmul_rn(t, t);
                    acc[k][4] += t;
                    acc[k][5] = fma(t, t, acc[k][5]);
                    acc[k][6] = fma(q, t, acc[k][6]);
                    acc[k][7] = fma(q, q, acc[k][7]);
                    a -= alo[k];
                    b -= ahi[k];
                }
                const double p = __dmul_rn(a, b);
                acc[k][0] = fma(a, b, acc[k][0]);
                acc[k][1] = fma(a, p, acc[k][1]);
                acc[k][2] = fma(b, p, acc[k][2]);
                acc[k][3] = fma(p, p, acc[k][3]);
            }
        }
    }
    double *dst = part + (o * nchunks + c) * NSL * (int64_t)npairs;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int q = tid + k * BLK;
        if (q < npairs) {
#pragma unroll
            for (int j = 0; j < NSL; j++) dst[j * npairs + q] = acc[k][j];
        }
    }
    if (tid < L) parte[(o * nchunks + c) * L + tid] = e;
}

// one thread per (slot, pair): adds the chunks in ascending order and writes the sum to its place; the threads of slot 0 that
// hold the first diagonal also fold `first`.  nsl = 4 or 8 slots; tpow was zeroed before the launch.
__global__ __launch_bounds__(BLK) void k_p4_fold(int64_t nchunks, int L, int nsl, const double *__restrict__ part,
                                                 const double *__restrict__ parte, double *__restrict__ first, double *__restrict__ s11,
                                                 double *__restrict__ s21, double *__restrict__ s22, double *__restrict__ tpow)
{
    const int npairs = n_pairs(L);
    const int idx = blockIdx.x * BLK + threadIdx.x;
    const int64_t o = blockIdx.y;
    if (idx >= nsl * npairs) return;
    const int slot = idx / npairs, q = idx - slot * npairs;
    const int64_t step = (int64_t)nsl * npairs;
    const double *src = part + o * nchunks * step + idx;
    double v = 0.0;
#pragma unroll 8
    for (int64_t c = 0; c < nchunks; c++) v += src[c * step];
    int lo, hi;
    pair_of(q, L, lo, hi);
    const int64_t LL = (int64_t)L * L, mat = o * LL, up = mat + lo * L + hi, down = mat + hi * L + lo;
    if (slot == 0) { s11[up] = v; s11[down] = v; }
    else if (slot == 1) s21[up] = v;
    else if (slot == 2) { if (lo < hi) s21[down] = v; }         // on the diagonal both are the sum of d^3: written once, by slot 1
    else if (slot == 3) { s22[up] = v; s22[down] = v; }
    else if (lo < hi) tpow[(o * NS + (slot - NS)) * LL + lo * L + hi] = v;
    if (idx < L) {                                              // slot 0, the first diagonal (it has L pairs: npairs >= L)
        double e = 0.0;
        for (int64_t c = 0; c < nchunks; c++) e += parte[(o * nchunks + c) * L + idx];
        first[o * L + idx] = e;
    }
}

}  // namespace

extern "C" int bluest_pilot_moments4(int64_t N, int L, int n_out, const double *values, const double *shift, double *first, double *s11,
                                     double *s21, double *s22, double *tpow, void *stream)
{
    if (L < 1 || L > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "L=%d out of range (1..%d)", L, BLUEST_MAX_MODELS);
    if (n_out < 1 || n_out > BLUEST_PILOT_MAX_OUTPUTS)
        return fail(BLUEST_ERR_ARG, "n_out=%d out of range (1..%d)", n_out, BLUEST_PILOT_MAX_OUTPUTS);
    if (N < 1) return fail(BLUEST_ERR_ARG, "N=%lld: at least one sample is needed", (long long)N);
    const int64_t nchunks = (N - 1) / CHUNK + 1;
    if (nchunks > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "N=%lld: more than 2^31 - 1 chunks of %d samples", (long long)N, CHUNK);
    if (!values || !first || !s11 || !s21 || !s22) return fail(BLUEST_ERR_ARG, "null pointer");
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool diff = tpow != nullptr, staged = !on_device(values);
    const int npairs = n_pairs(L);
    const size_t in_bytes = (size_t)n_out * (size_t)N * L * 8, mat = (size_t)n_out * L * L * 8, vec = (size_t)n_out * L * 8;
    DeviceArena arena;
    const int nsl = diff ? 2 * NS : NS;
    const size_t o_in = arena.take(staged ? in_bytes : 0), o_sh = arena.take(shift ? vec : 0),
                 o_part = arena.take((size_t)n_out * nchunks * nsl * npairs * 8), o_pe = arena.take((size_t)n_out * nchunks * L * 8),
                 o_first = arena.take(vec), o_11 = arena.take(mat), o_21 = arena.take(mat), o_22 = arena.take(mat),
                 o_tp = arena.take(diff ? NS * mat : 0);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_in = values;
    if (staged) {
        HIP_TRY(hipMemcpyAsync(dv + o_in, values, in_bytes, hipMemcpyHostToDevice, st));
        d_in = (const double *)(dv + o_in);
    }
    const double *d_sh = d_in;                                  // a null shift: the first sample, where it lies
    int64_t sh_stride = N * (int64_t)L;
    if (shift) {
        HIP_TRY(hipMemcpyAsync(dv + o_sh, shift, vec, hipMemcpyHostToDevice, st));
        d_sh = (const double *)(dv + o_sh);
        sh_stride = L;
    }
    double *d_part = (double *)(dv + o_part), *d_pe = (double *)(dv + o_pe), *d_first = (double *)(dv + o_first);
    double *d_11 = (double *)(dv + o_11), *d_21 = (double *)(dv + o_21), *d_22 = (double *)(dv + o_22);
    double *d_tp = diff ? (double *)(dv + o_tp) : nullptr;
    const dim3 g1((unsigned)nchunks, (unsigned)n_out), g2((unsigned)((nsl * npairs + BLK - 1) / BLK), (unsigned)n_out);
    const size_t lds = (size_t)CHUNK * L * 8;
    if (diff) {
        HIP_TRY(hipMemsetAsync(d_tp, 0, NS * mat, st));
        hipLaunchKernelGGL(k_p4_partial<true>, g1, dim3(BLK), lds, st, N, L, d_in, d_sh, sh_stride, d_part, d_pe);
    } else {
        hipLaunchKernelGGL(k_p4_partial<false>, g1, dim3(BLK), lds, st, N, L, d_in, d_sh, sh_stride, d_part, d_pe);
    }
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_p4_fold, g2, dim3(BLK), 0, st, nchunks, L, nsl, (const double *)d_part, (const double *)d_pe, d_first, d_11, d_21,
                       d_22, d_tp);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(first, d_first, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s11, d_11, mat, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s21, d_21, mat, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(s22, d_22, mat, hipMemcpyDeviceToHost, st));
    if (diff) HIP_TRY(hipMemcpyAsync(tpow, d_tp, NS * mat, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

// field_pilot.hip -- Part 17 of include/bluest_hip.h: per pair of models the first sample's value and the shifted sums, over the
// pilot samples, of the per-sample centred inner product q_s(i, j) = sum_c w_c x_i[c] x_j[c] and of the per-sample norm r_s(i, j)
// of the centred explicit difference: what the standard errors of a field's pilot covariances and MLMC variances are made of.
// The reduction runs over the components INSIDE a sample first and over the samples second, so nothing of bluest_field_stats
// (which adds over samples and components together) can be reused but its LDS layout.  No atomics, nothing sized by the device:
// the results are functions of the inputs and of BLUEST_FIELD_STRIP and BLUEST_PILOT_CHUNK only.
//
// Per run of whole chunks (a run is what fits the staging budget and the scratch limit), in stream order:
//   k_fp_strip   1-D grid over (sub-block of sb samples, strip of BLUEST_FIELD_STRIP components).  The workgroup walks its strip
//                in column blocks of CB components: it stages sb samples x L models x CB components, the L x CB centre values and
//                the CB weights in LDS -- read from memory in runs along c -- and every thread keeps the fma chains of its
//                (sample, pair) items in registers across the column blocks: one chain per item and strip, no join between threads.
//                Consecutive threads take consecutive pairs of pilot.hip's wrapped diagonals, so a half-wave reads consecutive
//                models; the odd row stride CB + 1 keeps them on different banks.  At the end the thread writes its chains:
//                scratch [sample][strip][slot][pair], slot 0 = q, slot 1 = r.
//   k_fp_join    only with more than one strip: a thread per (sample, slot, pair) adds the strips in ascending order.
//   (run 0)      the joined values of sample 0 are copied aside: q_0 and r_0, the shift of every later run.
//   k_fp_chunk   a thread per (chunk, slot, pair): u = q_s - q_0, s1 = s1 + u, s2 = fma(u, u, s2) over the chunk's samples.
// and at the end k_fp_total, a thread per (slot, pair): the chunks in ascending order, mirrored into the six matrices.
// sb and CB follow (L, d) alone (fp_shape): wide L takes one sample and short column blocks, narrow L many samples, d < 64 column
// blocks no wider than d.  They shape the launch, not the order.
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
constexpr int CHUNK = BLUEST_PILOT_CHUNK;
constexpr int STRIP = BLUEST_FIELD_STRIP;
constexpr int KMAX = (BLUEST_MAX_MODELS * (BLUEST_MAX_MODELS + 1) / 2 + BLK - 1) / BLK;     // (sample, pair) items per thread: 9
constexpr int CB_MAX = 64;
constexpr size_t LDS_LIMIT = 32 * 1024;            // per workgroup: five workgroups share a compute unit's 160 KiB
static_assert(CB_MAX <= BLK && STRIP % CB_MAX == 0, "a column block is staged by one pass of the workgroup and never straddles a strip");

std::atomic<int64_t> g_scratch_bytes{BLUEST_FIELD_PILOT_SCRATCH_BYTES};

struct PShape {
    int64_t N, d, nstrips;
    int L, npairs, ncols;           // ncols: (slot, pair) values per sample and strip
    int sb, CB, cb_shift, STR;      // samples per sub-block; components per column block (a power of two); LDS row stride CB + 1
};

size_t fp_lds_doubles(int L, int sb, int CB) { return (size_t)(sb + 1) * L * (CB + 1) + CB; }

// the launch shape of (L, d): about four items per thread, the widest column block that fits, then more samples where d is small
void fp_shape(PShape &sh)
{
    const int L = sh.L, most = KMAX * BLK / sh.npairs;
    int cap = 1;
    while (cap < CB_MAX && cap < sh.d) cap *= 2;
    int sb = std::max(1, std::min(most, (4 * BLK + sh.npairs - 1) / sh.npairs)), CB = cap;
    while (CB > 8 && fp_lds_doubles(L, sb, CB) * 8 > LDS_LIMIT) CB /= 2;
    while (sb > 1 && fp_lds_doubles(L, sb, CB) * 8 > LDS_LIMIT) sb--;
    while (CB > 1 && fp_lds_doubles(L, sb, CB) * 8 > LDS_LIMIT) CB /= 2;
    if (CB == cap)                                                     // d < 64: one short block per sample, so more samples per workgroup
        while (sb < most && sb < 4 * CHUNK && fp_lds_doubles(L, sb + 1, CB) * 8 <= LDS_LIMIT) sb++;
    sh.sb = sb; sh.CB = CB; sh.STR = CB + 1;
    sh.cb_shift = 0;
    while ((1 << sh.cb_shift) < CB) sh.cb_shift++;
}

// values: sample 0 of the run; nsamp: samples of the run; grid: ceil(nsamp / sb) * nstrips
template <bool DIFF>
__global__ __launch_bounds__(BLK) void k_fp_strip(PShape sh, int64_t nsamp, const double *__restrict__ values, const double *__restrict__ w,
                                                  const double *__restrict__ centre, double *__restrict__ scratch)
{
    extern __shared__ double lds[];
    const int tid = threadIdx.x, L = sh.L, sb = sh.sb, CB = sh.CB, STR = sh.STR, npairs = sh.npairs;
    const int64_t d = sh.d, b = blockIdx.x, sub = b / sh.nstrips, strip = b - sub * sh.nstrips;
    const int64_t s0 = sub * sb;
    const int ns = (int)min((int64_t)sb, nsamp - s0), nitems = ns * npairs, mcount = (nitems + BLK - 1) / BLK;
    const int64_t c_begin = strip * STRIP, c_end = min(d, c_begin + STRIP);
    double *Y = lds, *CE = lds + (size_t)sb * L * STR, *W = CE + (size_t)L * STR;
    const double *src = values + s0 * L * d;

    int ybase[KMAX], at_lo[KMAX], at_hi[KMAX];                         // LDS offsets: the item's sample, the pair's two models
    double p[KMAX], r[KMAX];
#pragma unroll
    for (int m = 0; m < KMAX; m++) {
        const int v = tid + m * BLK;
        int s = 0, lo = 0, hi = 0;
        if (v < nitems) {
            s = v / npairs;
            pair_of(v - s * npairs, L, lo, hi);
        }
        ybase[m] = s * L * STR;
        at_lo[m] = lo * STR;
        at_hi[m] = hi * STR;
        p[m] = r[m] = 0.0;
    }

    for (int64_t cb = c_begin; cb < c_end; cb += CB) {
        const int cw = (int)min((int64_t)CB, c_end - cb);
        __syncthreads();                                               // every read of the last column block is done
        for (int t = tid; t < ((ns * L) << sh.cb_shift); t += BLK) {   // runs of cw components along c, the fastest index
            const int row = t >> sh.cb_shift, c = t & (CB - 1);
            if (c < cw) Y[row * STR + c] = src[(int64_t)row * d + cb + c];
        }
        for (int t = tid; t < (L << sh.cb_shift); t += BLK) {
            const int row = t >> sh.cb_shift, c = t & (CB - 1);
            if (c < cw) CE[row * STR + c] = centre[(int64_t)row * d + cb + c];
        }
        if (tid < cw) W[tid] = w[cb + tid];
        __syncthreads();
        for (int c = 0; c < cw; c++) {
            const double wc = W[c];
#pragma unroll
            for (int m = 0; m < KMAX; m++) {
                if (m < mcount) {
                    const double yi = Y[ybase[m] + at_lo[m] + c], yj = Y[ybase[m] + at_hi[m] + c];
                    const double ci = CE[at_lo[m] + c], cj = CE[at_hi[m] + c];
                    const double a = yi - ci, bb = yj - cj;
                    p[m] = fma(wc * a, bb, p[m]);
                    if (DIFF) {
                        const double t = (yi - yj) - (ci - cj);
                        r[m] = fma(wc * t, t, r[m]);
                    }
                }
            }
        }
    }

#pragma unroll
    for (int m = 0; m < KMAX; m++) {
        const int v = tid + m * BLK;
        if (v < nitems) {
            const int s = v / npairs, pr = v - s * npairs;
            double *dst = scratch + ((s0 + s) * sh.nstrips + strip) * sh.ncols + pr;
            dst[0] = p[m];
            if (DIFF) dst[npairs] = r[m];
        }
    }
}

// joined [sample][col] = the strips of scratch [sample][strip][col] in ascending order from +0.0
__global__ __launch_bounds__(BLK) void k_fp_join(PShape sh, int64_t nsamp, const double *__restrict__ scratch, double *__restrict__ joined)
{
    const int64_t v = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (v >= nsamp * sh.ncols) return;
    const int64_t s = v / sh.ncols, col = v - s * sh.ncols;
    const double *src = scratch + s * sh.nstrips * sh.ncols + col;
    double q = 0.0;
    for (int64_t k = 0; k < sh.nstrips; k++) q += src[k * sh.ncols];
    joined[v] = q;
}

// grid (chunks of the run, column blocks); part: [chunk][s1 | s2][col]
__global__ __launch_bounds__(BLK) void k_fp_chunk(PShape sh, int64_t chunk0, int64_t nsamp, const double *__restrict__ joined,
                                                  const double *__restrict__ first, double *__restrict__ part)
{
    const int col = blockIdx.y * BLK + threadIdx.x;
    if (col >= sh.ncols) return;
    const int64_t local = blockIdx.x;
    const int ns = (int)min((int64_t)CHUNK, nsamp - local * CHUNK);
    const double *src = joined + local * CHUNK * sh.ncols + col;
    const double q0 = first[col];
    double s1 = 0.0, s2 = 0.0;
    for (int s = 0; s < ns; s++) {
        const double u = src[(int64_t)s * sh.ncols] - q0;
        s1 = s1 + u;
        s2 = fma(u, u, s2);
    }
    double *dst = part + (chunk0 + local) * 2 * sh.ncols + col;
    dst[0] = s1;
    dst[sh.ncols] = s2;
}

// out: [qfirst | qs1 | qs2 | rfirst | rs1 | rs2][L x L], set to zero before the launch
__global__ __launch_bounds__(BLK) void k_fp_total(PShape sh, int64_t nchunks, const double *__restrict__ first, const double *__restrict__ part,
                                                  double *__restrict__ out)
{
    const int col = blockIdx.x * BLK + threadIdx.x;
    if (col >= sh.ncols) return;
    double s1 = 0.0, s2 = 0.0;
    for (int64_t k = 0; k < nchunks; k++) {
        s1 += part[k * 2 * sh.ncols + col];
        s2 += part[(k * 2 + 1) * sh.ncols + col];
    }
    const int L = sh.L, slot = col / sh.npairs;
    int lo, hi;
    pair_of(col - slot * sh.npairs, L, lo, hi);
    double *dst = out + (size_t)slot * 3 * L * L;
    if (slot == 1 && lo == hi) return;                                 // r lives at i < j
    dst[lo * L + hi] = first[col];
    dst[L * L + lo * L + hi] = s1;
    dst[2 * L * L + lo * L + hi] = s2;
    if (slot == 0) {
        dst[hi * L + lo] = first[col];
        dst[L * L + hi * L + lo] = s1;
        dst[2 * L * L + hi * L + lo] = s2;
    }
}

}  // namespace

extern "C" int bluest_field_pilot_scratch(int64_t bytes, int64_t *previous)
{
    if (bytes < 0) return fail(BLUEST_ERR_ARG, "bytes=%lld: the scratch limit cannot be negative (0 leaves it as it is)", (long long)bytes);
    if (previous) *previous = g_scratch_bytes.load();
    if (bytes > 0) g_scratch_bytes.store(bytes);
    return BLUEST_OK;
}

extern "C" int bluest_field_pilot_moments(int64_t N, int L, int64_t d, const double *values, const double *w, const double *centre,
                                          double *qfirst, double *qs1, double *qs2, double *rfirst, double *rs1, double *rs2, void *stream)
{
    if (L < 1 || L > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "L=%d out of range (1..%d)", L, BLUEST_MAX_MODELS);
    if (d < 1) return fail(BLUEST_ERR_ARG, "d=%lld: at least one component is needed", (long long)d);
    if (N < 1) return fail(BLUEST_ERR_ARG, "N=%lld: at least one sample is needed", (long long)N);
    if (!values || !w || !centre || !qfirst || !qs1 || !qs2) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((uintptr_t)values & 7) return fail(BLUEST_ERR_ARG, "values is not 8-byte aligned");
    const int nr = (rfirst != nullptr) + (rs1 != nullptr) + (rs2 != nullptr);
    if (nr != 0 && nr != 3) return fail(BLUEST_ERR_ARG, "rfirst, rs1 and rs2 must all be given or all be null");
    for (int64_t c = 0; c < d; c++)
        if (!(w[c] >= 0.0) || std::isinf(w[c])) return fail(BLUEST_ERR_ARG, "w[%lld]=%g: the weights must be finite and >= 0", (long long)c, w[c]);
    const bool diff = nr == 3;
    PShape sh;
    sh.N = N; sh.d = d; sh.L = L;
    sh.nstrips = (d - 1) / STRIP + 1;
    sh.npairs = n_pairs(L);
    sh.ncols = (diff ? 2 : 1) * sh.npairs;
    fp_shape(sh);
    const int64_t nchunks = (N - 1) / CHUNK + 1;
    if ((double)L * (double)d > 2147483647.0 || nchunks > 0x7fffffffLL)
        return fail(BLUEST_ERR_ARG, "N=%lld, L=%d, d=%lld: more than 2^31 - 1 (model, component) values per sample or chunks of %d samples",
                    (long long)N, L, (long long)d, CHUNK);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool staged = !on_device(values);

    // runs of whole chunks: what the staging budget (host input) and the scratch limit allow, at least one chunk, and no more
    // workgroups than a 1-D grid takes
    const size_t sample_bytes = (size_t)L * d * 8, sample_scratch = (size_t)(sh.nstrips + (sh.nstrips > 1 ? 1 : 0)) * sh.ncols * 8;
    int64_t run_chunks = std::max<int64_t>(1, g_scratch_bytes.load() / (int64_t)(sample_scratch * CHUNK));
    if (staged) run_chunks = std::min(run_chunks, std::max<int64_t>(1, slab_budget() / (int64_t)(sample_bytes * CHUNK)));
    run_chunks = std::min(run_chunks, nchunks);
    while (run_chunks > 1 && (double)(run_chunks * CHUNK / sh.sb + 1) * (double)sh.nstrips > 2147483647.0) run_chunks /= 2;
    if ((double)(CHUNK / sh.sb + 1) * (double)sh.nstrips > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "d=%lld: more than 2^31 - 1 (sub-block, strip) workgroups per chunk", (long long)d);
    const int64_t run_samples = std::min<int64_t>(N, run_chunks * CHUNK);

    const size_t mat = (size_t)L * L * 8, vec = (size_t)L * d * 8;
    DeviceArena arena;
    const size_t o_in = arena.take(staged ? (size_t)run_samples * sample_bytes : 0), o_w = arena.take((size_t)d * 8), o_ce = arena.take(vec),
                 o_scr = arena.take((size_t)run_samples * sh.nstrips * sh.ncols * 8),
                 o_join = arena.take(sh.nstrips > 1 ? (size_t)run_samples * sh.ncols * 8 : 0), o_first = arena.take((size_t)sh.ncols * 8),
                 o_part = arena.take((size_t)nchunks * 2 * sh.ncols * 8), o_out = arena.take(6 * mat);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    double *d_w = (double *)(dv + o_w), *d_ce = (double *)(dv + o_ce), *d_scr = (double *)(dv + o_scr);
    double *d_join = sh.nstrips > 1 ? (double *)(dv + o_join) : d_scr, *d_first = (double *)(dv + o_first);
    double *d_part = (double *)(dv + o_part), *d_out = (double *)(dv + o_out);
    HIP_TRY(hipMemcpyAsync(d_w, w, (size_t)d * 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(d_ce, centre, vec, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(d_out, 0, 6 * mat, st));

    const size_t lds = fp_lds_doubles(L, sh.sb, sh.CB) * 8;
    for (int64_t c0 = 0; c0 < nchunks; c0 += run_chunks) {
        const int64_t nc = std::min(run_chunks, nchunks - c0), nsamp = std::min<int64_t>(N - c0 * CHUNK, nc * CHUNK);
        const double *d_in = values + c0 * CHUNK * L * d;
        if (staged) {
            HIP_TRY(hipMemcpyAsync(dv + o_in, d_in, (size_t)nsamp * sample_bytes, hipMemcpyHostToDevice, st));
            d_in = (const double *)(dv + o_in);                         // in stream order: the next run's copy waits for the kernel
        }
        const dim3 grid((unsigned)(((nsamp - 1) / sh.sb + 1) * sh.nstrips));
        if (diff) hipLaunchKernelGGL(k_fp_strip<true>, grid, dim3(BLK), lds, st, sh, nsamp, d_in, (const double *)d_w, (const double *)d_ce, d_scr);
        else hipLaunchKernelGGL(k_fp_strip<false>, grid, dim3(BLK), lds, st, sh, nsamp, d_in, (const double *)d_w, (const double *)d_ce, d_scr);
        HIP_TRY(hipGetLastError());
        if (sh.nstrips > 1) {
            const dim3 gj((unsigned)((nsamp * sh.ncols - 1) / BLK + 1));
            hipLaunchKernelGGL(k_fp_join, gj, dim3(BLK), 0, st, sh, nsamp, (const double *)d_scr, d_join);
            HIP_TRY(hipGetLastError());
        }
        if (c0 == 0) HIP_TRY(hipMemcpyAsync(d_first, d_join, (size_t)sh.ncols * 8, hipMemcpyDeviceToDevice, st));
        const dim3 gc((unsigned)nc, (unsigned)((sh.ncols - 1) / BLK + 1));
        hipLaunchKernelGGL(k_fp_chunk, gc, dim3(BLK), 0, st, sh, c0, nsamp, (const double *)d_join, (const double *)d_first, d_part);
        HIP_TRY(hipGetLastError());
    }
    hipLaunchKernelGGL(k_fp_total, dim3((unsigned)((sh.ncols - 1) / BLK + 1)), dim3(BLK), 0, st, sh, nchunks, (const double *)d_first,
                       (const double *)d_part, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(qfirst, d_out, mat, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(qs1, d_out + (size_t)L * L, mat, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(qs2, d_out + 2 * (size_t)L * L, mat, hipMemcpyDeviceToHost, st));
    if (diff) {
        HIP_TRY(hipMemcpyAsync(rfirst, d_out + 3 * (size_t)L * L, mat, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(rs1, d_out + 4 * (size_t)L * L, mat, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(rs2, d_out + 5 * (size_t)L * L, mat, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

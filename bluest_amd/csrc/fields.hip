// fields.hip -- Part 12 of include/bluest_hip.h: Parts 10 and 11 for outputs that are vectors of d components with a diagonal
// inner product <a, b> = sum_c w_c a_c b_c (bluest/blue_fn.py:147-167 with the inner products of get_models_inner_products, one
// Python call per pair and sample).  No atomics, nothing sized by the device: the results are functions of the inputs and of
// BLUEST_PILOT_CHUNK, BLUEST_FIELD_TILE and BLUEST_GSUM_CHUNK only.
//
// bluest_field_stats, three launches (plus one k_field_partial per further slab of staged host data):
//   k_field_partial     1-D grid over (chunk of BLUEST_PILOT_CHUNK samples, block of TB component tiles).  The workgroup stages
//                       sub-blocks of a few samples x L models x 8 TB components in LDS -- read from memory in runs along c, the
//                       fastest index of `values` -- and keeps its sums in registers across the sub-blocks.  A thread owns
//                       pairs of one tile, the pairs numbered along pilot.hip's wrapped diagonals, and walks s ascending, then
//                       c ascending inside the tile.  TB (a power of two, at most 16) only shapes the workgroup: a narrow L has
//                       few pairs, so a workgroup takes several tiles side by side, which also makes the runs along c longer.
//                       The order of the additions does not depend on it.
//                       LDS image: [tile of the block][sample of the sub-block][model][8 components + 1 pad]; the odd stride
//                       of 9 doubles keeps 32 consecutive models on 32 different bank pairs for ds_read_b64.
//   k_field_fold_pairs  a wave per pair: per chunk in ascending order, lane l adds the tiles l, l + 64, ... in ascending order,
//                       the lanes are joined by the fixed tree of Part 11, and the chunk's value is added to the total.
//   k_field_fold_comp   a thread per (model or pair, component): the chunks in ascending order.
// bluest_field_sums, two or three launches (plus one k_fsum_partial per further slab):
//   k_fsum_partial      grid (chunk, column block) over a host-built table of chunks: a thread per column-component of the
//                       segment's rows of sizes[s] d contiguous doubles (coalesced), the rows of the chunk in the order of Part 11.
//   k_fsum_fold         grid (segment, block of 64 column-components): wave g = 0..3 computes the lane sums l = g, g + 4, ... of
//                       Part 11 step 3 for its 64 columns into LDS (coalesced along the columns), then the tree runs over LDS.
//   k_fsum_mu           a thread per (repeat, component): the fma chain over the repeat's columns in ascending order.
// The segments' checks, the slabs of staged host data, the chunk table and the slab loop of bluest_field_sums are those of
// staging.hpp; bluest_field_stats has one array and cuts it into slabs of whole chunks itself.
#include "staging.hpp"
#include "field_partials.hpp"

namespace {

using bluest_partials::FChunk;

constexpr int BLK = 256;
constexpr int CHUNK = BLUEST_PILOT_CHUNK;
constexpr int TILE = BLUEST_FIELD_TILE;
constexpr int STR = TILE + 1;                       // doubles from model i to model i + 1 in LDS
constexpr int KMAX = (BLUEST_MAX_MODELS * (BLUEST_MAX_MODELS + 1) / 2 + BLK - 1) / BLK;     // pairs per thread: 9
constexpr int TB_MAX = 16;
constexpr int EMAX = 8;                             // (model, component) sums per thread: L * TILE * TB <= EMAX * BLK
constexpr size_t LDS_BYTES = 64 * 1024;
static_assert(TILE == 8, "the shifts and masks below take a tile of 8 components");
static_assert((size_t)BLUEST_MAX_MODELS * STR * sizeof(double) <= LDS_BYTES, "one sample of the widest problem must fit the LDS");

// tiles per workgroup: the largest power of two with npairs * TB <= KMAX * BLK and L * TILE * TB <= EMAX * BLK, at most TB_MAX
// and no more than it takes to cover the ntiles tiles there are
int tiles_per_block(int L, int64_t ntiles)
{
    int tb = 1;
    while (tb < TB_MAX && tb < ntiles && n_pairs(L) * 2 * tb <= KMAX * BLK && L * TILE * 2 * tb <= EMAX * BLK) tb *= 2;
    return tb;
}

struct FieldShape {
    int64_t N, d, nchunks, ntiles, nblocks;         // nblocks: workgroups per chunk = ceil(ntiles / TB)
    int L, TB, tb_shift, sb;                        // sb: samples per sub-block
};

// partp: [slot][pair][chunk][tile], slot 0 = sum w y_lo y_hi, with DIFF slot 1 = sum w (y_lo - y_hi)^2
// parte: [chunk][model][d] = sum y_i[c];  partd (DIFF): [chunk][pair][d] = sum (y_lo[c] - y_hi[c]), pairs lo < hi only
template <bool DIFF, bool FULL>
__device__ __forceinline__ void field_partial_body(const FieldShape &sh, int64_t chunk, int64_t blk, int ns, const double *__restrict__ src,
                                                   const double *__restrict__ w, double *__restrict__ partp,
                                                   double *__restrict__ parte, double *__restrict__ partd, double *tile)
{
    const int tid = threadIdx.x;
    const int L = sh.L, TB = sh.TB, sb = sh.sb;
    const int64_t d = sh.d;
    const int64_t cb0 = blk * TB * TILE;                               // first component of the block
    const int bw = (int)min((int64_t)TB * TILE, d - cb0);              // components of the block
    const int bwp = TB * TILE, bshift = sh.tb_shift + 3;               // padded width, a power of two
    // the thread's tile and pairs: BLK / TB consecutive threads share a tile, thread j of them owns the pairs j, j + BLK / TB, ...
    const int npairs = n_pairs(L), G = BLK >> sh.tb_shift, tb = tid >> (8 - sh.tb_shift), pl = tid & (G - 1);
    const int kcount = (npairs + G - 1) / G;
    const int tw = FULL ? TILE : max(0, min(TILE, bw - tb * TILE));    // components of the thread's tile
    const int at_tile = tb * sb * L * STR;

    int at_lo[KMAX], at_hi[KMAX];                                      // LDS offsets of the pair's two models
    double p[KMAX], q[KMAX], r[KMAX][TILE], wc[TILE];
#pragma unroll
    for (int c = 0; c < TILE; c++) wc[c] = c < tw ? w[cb0 + tb * TILE + c] : 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int pr = pl + k * G;
        int lo = 0, hi = 0;
        if (pr < npairs) pair_of(pr, L, lo, hi);
        at_lo[k] = at_tile + lo * STR;
        at_hi[k] = at_tile + hi * STR;
        p[k] = q[k] = 0.0;
#pragma unroll
        for (int c = 0; c < TILE; c++) r[k][c] = 0.0;
    }
    int at_e[EMAX];
    double e[EMAX];
#pragma unroll
    for (int m = 0; m < EMAX; m++) {
        const int v = tid + m * BLK, i = v >> bshift, c = v & (bwp - 1);
        at_e[m] = (i < L && c < bw) ? (((c >> 3) * sb * L + i) * STR + (c & 7)) : -1;
        e[m] = 0.0;
    }

    for (int sub = 0; sub < ns; sub += sb) {
        const int nsb = min(sb, ns - sub), rows = nsb * L;
        __syncthreads();                                               // every read of the last sub-block is done
        for (int t = tid; t < (rows << bshift); t += BLK) {            // runs of bw components along c, the fastest index
            const int row = t >> bshift, c = t & (bwp - 1);
            if (FULL || c < bw) tile[((c >> 3) * sb * L + row) * STR + (c & 7)] = src[((int64_t)sub * L + row) * d + cb0 + c];
        }
        __syncthreads();
        for (int s = 0; s < nsb; s++) {
            const double *row = tile + s * L * STR;
#pragma unroll
            for (int m = 0; m < EMAX; m++)
                if (at_e[m] >= 0) e[m] += row[at_e[m]];
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                if (k < kcount) {
                    const double *ya = row + at_lo[k], *yb = row + at_hi[k];
#pragma unroll
                    for (int c = 0; c < TILE; c++) {
                        if (FULL || c < tw) {
                            const double a = ya[c], b = yb[c];
                            p[k] = fma(wc[c] * a, b, p[k]);
                            if (DIFF) {
                                const double dd = a - b;
                                r[k][c] += dd;
                                q[k] = fma(wc[c] * dd, dd, q[k]);
                            }
                        }
                    }
                }
            }
        }
    }

    const int64_t t = blk * TB + tb;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int pr = pl + k * G;
        if (pr < npairs && tw > 0) {
            partp[((int64_t)pr * sh.nchunks + chunk) * sh.ntiles + t] = p[k];
            if (DIFF) {
                partp[(((int64_t)npairs + pr) * sh.nchunks + chunk) * sh.ntiles + t] = q[k];
                if (at_lo[k] != at_hi[k]) {
                    double *dst = partd + (chunk * npairs + pr) * d + t * TILE;
#pragma unroll
                    for (int c = 0; c < TILE; c++)
                        if (FULL || c < tw) dst[c] = r[k][c];
                }
            }
        }
    }
#pragma unroll
    for (int m = 0; m < EMAX; m++) {
        const int v = tid + m * BLK;
        if (at_e[m] >= 0) parte[(chunk * L + (v >> bshift)) * d + cb0 + (v & (bwp - 1))] = e[m];
    }
}

// values: sample 0 of chunk `chunk0` (the slab's first); grid: (chunks of the slab) * nblocks
template <bool DIFF>
__global__ __launch_bounds__(BLK) void k_field_partial(FieldShape sh, int64_t chunk0, const double *__restrict__ values,
                                                       const double *__restrict__ w, double *__restrict__ partp,
                                                       double *__restrict__ parte, double *__restrict__ partd)
{
    extern __shared__ double tile[];
    const int64_t b = blockIdx.x, local = b / sh.nblocks, blk = b - local * sh.nblocks, chunk = chunk0 + local;
    const int ns = (int)min((int64_t)CHUNK, sh.N - chunk * CHUNK);
    const double *src = values + local * CHUNK * sh.L * sh.d;
    if ((blk + 1) * sh.TB * TILE <= sh.d) field_partial_body<DIFF, true>(sh, chunk, blk, ns, src, w, partp, parte, partd, tile);
    else field_partial_body<DIFF, false>(sh, chunk, blk, ns, src, w, partp, parte, partd, tile);
}

// one wave per pair; sumsd2 was set to zero before the launch
template <bool DIFF>
__global__ __launch_bounds__(BLK) void k_field_fold_pairs(FieldShape sh, const double *__restrict__ partp, double *__restrict__ sumsc,
                                                          double *__restrict__ sumsd2)
{
    const int L = sh.L, npairs = n_pairs(L), lane = threadIdx.x & 63;
    const int pr = blockIdx.x * (BLK / WAVE) + (threadIdx.x >> 6);
    if (pr >= npairs) return;                                          // whole waves leave
    double tot[2] = {0.0, 0.0};
#pragma unroll
    for (int slot = 0; slot < (DIFF ? 2 : 1); slot++) {
        const double *src = partp + ((int64_t)slot * npairs + pr) * sh.nchunks * sh.ntiles;
        for (int64_t c = 0; c < sh.nchunks; c++) {
            double acc = 0.0;
            for (int64_t t = lane; t < sh.ntiles; t += WAVE) acc += src[c * sh.ntiles + t];
            tot[slot] += wave_sum(acc);                                // lane 0's tree; every lane ends with the same bits
        }
    }
    if (lane != 0) return;
    int lo, hi;
    pair_of(pr, L, lo, hi);
    sumsc[lo * L + hi] = tot[0];
    sumsc[hi * L + lo] = tot[0];
    if (DIFF && lo < hi) sumsd2[lo * L + hi] = tot[1];
}

// grid (component block, row): row < L -> sumse[row], else pair number row - L (i < j, row-major) -> sumsd1; qmap[pair] = its
// wrapped-diagonal number
__global__ __launch_bounds__(BLK) void k_field_fold_comp(FieldShape sh, const int32_t *__restrict__ qmap, const double *__restrict__ parte,
                                                         const double *__restrict__ partd, double *__restrict__ sumse,
                                                         double *__restrict__ sumsd1)
{
    const int64_t c = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (c >= sh.d) return;
    const int row = blockIdx.y, L = sh.L;
    const double *src;
    int64_t step;
    double *dst;
    if (row < L) {
        src = parte + (int64_t)row * sh.d + c;
        step = (int64_t)L * sh.d;
        dst = sumse + (int64_t)row * sh.d + c;
    } else {
        src = partd + (int64_t)qmap[row - L] * sh.d + c;
        step = (int64_t)n_pairs(L) * sh.d;
        dst = sumsd1 + (int64_t)(row - L) * sh.d + c;
    }
    double acc = 0.0;
    for (int64_t k = 0; k < sh.nchunks; k++) acc += src[k * step];
    *dst = acc;
}

// ---- bluest_field_sums ---------------------------------------------------------------------------------------------------------
constexpr int FOLD_COLS = 64;

struct FSeg {
    int64_t part;           // first chunk's partial sums
    int64_t nchunks;
    int64_t W, flat0;       // the segment's column-components are sums[flat0 .. flat0 + W)
};

__global__ __launch_bounds__(BLK) void k_fsum_partial(const FChunk *__restrict__ table, double *__restrict__ part)
{
    const FChunk ch = table[blockIdx.x];
    for (int64_t col = (int64_t)blockIdx.y * BLK + threadIdx.x; col < ch.W; col += (int64_t)gridDim.y * BLK) {
        const double *src = ch.src + col;
        double q[CLASSES];
#pragma unroll
        for (int k = 0; k < CLASSES; k++) {
            q[k] = 0.0;
            const int r1 = min((k + 1) * CLASS_ROWS, ch.rows);
            if (r1 - k * CLASS_ROWS == CLASS_ROWS) {
#pragma unroll
                for (int r = 0; r < CLASS_ROWS; r++) q[k] += src[(int64_t)(k * CLASS_ROWS + r) * ch.W];
            } else {
                for (int r = k * CLASS_ROWS; r < r1; r++) q[k] += src[(int64_t)r * ch.W];
            }
        }
        part[ch.part + col] = class_tree(q);
    }
}

__global__ __launch_bounds__(BLK) void k_fsum_fold(const FSeg *__restrict__ segs, const double *__restrict__ part, double *__restrict__ sums)
{
    __shared__ double p[WAVE][FOLD_COLS];
    const FSeg sg = segs[blockIdx.x];
    const int tid = threadIdx.x, g = tid >> 6, j = tid & 63;
    for (int64_t col0 = (int64_t)blockIdx.y * FOLD_COLS; col0 < sg.W; col0 += (int64_t)gridDim.y * FOLD_COLS) {
        const int64_t col = col0 + j;
        for (int l = g; l < WAVE; l += BLK / WAVE) {
            double acc = 0.0;
            if (col < sg.W)
                for (int64_t c = l; c < sg.nchunks; c += WAVE) acc += part[sg.part + c * sg.W + col];
            p[l][j] = acc;
        }
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) {                       // lane l < off takes p_l + p_(l + off)
            for (int v = tid; v < off * FOLD_COLS; v += BLK) p[v >> 6][v & 63] += p[(v >> 6) + off][v & 63];
            __syncthreads();
        }
        if (tid < FOLD_COLS && col < sg.W) sums[sg.flat0 + col] = p[0][tid];
        __syncthreads();
    }
}

// grid (repeat, component block); cols[r], cols[r + 1]: the columns of repeat r
__global__ __launch_bounds__(BLK) void k_fsum_mu(int64_t d, const int64_t *__restrict__ cols, const double *__restrict__ weights,
                                                 const double *__restrict__ sums, double *__restrict__ mu)
{
    const int64_t r = blockIdx.x;
    for (int64_t c = (int64_t)blockIdx.y * BLK + threadIdx.x; c < d; c += (int64_t)gridDim.y * BLK) {
        double m = 0.0;
        for (int64_t t = cols[r]; t < cols[r + 1]; t++) m = fma(weights[t], sums[t * d + c], m);
        mu[r * d + c] = m;
    }
}

}  // namespace

hipError_t bluest_partials::launch_fsum_partial(const FChunk *table, size_t n, int64_t Wmax, double *part, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const dim3 grid((unsigned)n, (unsigned)std::min<int64_t>((Wmax + BLK - 1) / BLK, 65535));
    hipLaunchKernelGGL(k_fsum_partial, grid, dim3(BLK), 0, st, table, part);
    return hipGetLastError();
}

extern "C" int bluest_field_stats(int64_t N, int L, int64_t d, const double *values, const double *w, double *sumse, double *sumsc,
                                  double *sumsd1, double *sumsd2, void *stream)
{
    if (L < 1 || L > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "L=%d out of range (1..%d)", L, BLUEST_MAX_MODELS);
    if (d < 1) return fail(BLUEST_ERR_ARG, "d=%lld: at least one component is needed", (long long)d);
    if (N < 1) return fail(BLUEST_ERR_ARG, "N=%lld: at least one sample is needed", (long long)N);
    if (!values || !w || !sumse || !sumsc) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((sumsd1 == nullptr) != (sumsd2 == nullptr)) return fail(BLUEST_ERR_ARG, "sumsd1 and sumsd2 must both be given or both be null");
    for (int64_t c = 0; c < d; c++)
        if (!(w[c] >= 0.0) || std::isinf(w[c])) return fail(BLUEST_ERR_ARG, "w[%lld]=%g: the weights must be finite and >= 0", (long long)c, w[c]);
    FieldShape sh;
    sh.N = N; sh.d = d; sh.L = L;
    sh.nchunks = (N - 1) / CHUNK + 1;
    sh.ntiles = (d - 1) / TILE + 1;
    sh.TB = tiles_per_block(L, sh.ntiles);
    sh.tb_shift = 0;
    while ((1 << sh.tb_shift) < sh.TB) sh.tb_shift++;
    sh.nblocks = (sh.ntiles - 1) / sh.TB + 1;
    sh.sb = (int)std::min<size_t>(CHUNK, LDS_BYTES / ((size_t)sh.TB * L * STR * 8));
    const int npairs = n_pairs(L), P = L * (L - 1) / 2;
    if ((double)npairs * (double)d > 2147483647.0 || (double)sh.nchunks * (double)sh.nblocks > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "N=%lld, L=%d, d=%lld: more than 2^31 - 1 (pair, component) sums or (chunk, tile block) workgroups",
                    (long long)N, L, (long long)d);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const bool diff = sumsd1 != nullptr, staged = !on_device(values);

    // host input goes through one staging buffer in slabs of whole chunks; at least one chunk is always staged
    const size_t chunk_bytes = (size_t)CHUNK * L * d * 8;
    const int64_t slab_chunks = staged ? std::min<int64_t>(sh.nchunks, std::max<int64_t>(1, slab_budget() / (int64_t)chunk_bytes)) : sh.nchunks;
    const size_t mat = (size_t)L * L * 8, vec = (size_t)L * d * 8, dvec = (size_t)P * d * 8;
    DeviceArena arena;
    const size_t o_in = arena.take(staged ? (size_t)std::min<int64_t>(N, slab_chunks * CHUNK) * L * d * 8 : 0), o_w = arena.take((size_t)d * 8),
                 o_pp = arena.take((size_t)(diff ? 2 : 1) * npairs * sh.nchunks * sh.ntiles * 8), o_pe = arena.take((size_t)sh.nchunks * vec),
                 o_pd = arena.take(diff ? (size_t)sh.nchunks * npairs * d * 8 : 0), o_q = arena.take(diff ? (size_t)P * 4 : 0),
                 o_se = arena.take(vec), o_sc = arena.take(mat), o_d1 = arena.take(diff ? dvec : 0), o_d2 = arena.take(diff ? mat : 0);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    double *d_w = (double *)(dv + o_w), *d_pp = (double *)(dv + o_pp), *d_pe = (double *)(dv + o_pe), *d_pd = (double *)(dv + o_pd);
    double *d_se = (double *)(dv + o_se), *d_sc = (double *)(dv + o_sc), *d_d1 = (double *)(dv + o_d1), *d_d2 = (double *)(dv + o_d2);
    int32_t *d_q = (int32_t *)(dv + o_q);
    HIP_TRY(hipMemcpyAsync(d_w, w, (size_t)d * 8, hipMemcpyHostToDevice, st));
    std::vector<int32_t> qmap;
    if (diff) {
        qmap.reserve((size_t)P);
        for (int i = 0; i < L; i++)
            for (int j = i + 1; j < L; j++) qmap.push_back(pair_number(i, j, L));
        if (P > 0) HIP_TRY(hipMemcpyAsync(d_q, qmap.data(), (size_t)P * 4, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_d2, 0, mat, st));
    }
    const size_t lds = (size_t)sh.sb * sh.TB * L * STR * 8;
    for (int64_t c0 = 0; c0 < sh.nchunks; c0 += slab_chunks) {
        const int64_t nc = std::min(slab_chunks, sh.nchunks - c0);
        const double *d_in = values + c0 * CHUNK * L * d;
        if (staged) {
            const int64_t rows = std::min<int64_t>(N - c0 * CHUNK, nc * CHUNK);
            HIP_TRY(hipMemcpyAsync(dv + o_in, d_in, (size_t)rows * L * d * 8, hipMemcpyHostToDevice, st));
            d_in = (const double *)(dv + o_in);                         // in stream order: the next slab's copy waits for the kernel
        }
        const dim3 grid((unsigned)(nc * sh.nblocks));
        if (diff) hipLaunchKernelGGL(k_field_partial<true>, grid, dim3(BLK), lds, st, sh, c0, d_in, (const double *)d_w, d_pp, d_pe, d_pd);
        else hipLaunchKernelGGL(k_field_partial<false>, grid, dim3(BLK), lds, st, sh, c0, d_in, (const double *)d_w, d_pp, d_pe, d_pd);
        HIP_TRY(hipGetLastError());
    }
    const dim3 g2((unsigned)((npairs + BLK / WAVE - 1) / (BLK / WAVE)));
    if (diff) hipLaunchKernelGGL(k_field_fold_pairs<true>, g2, dim3(BLK), 0, st, sh, (const double *)d_pp, d_sc, d_d2);
    else hipLaunchKernelGGL(k_field_fold_pairs<false>, g2, dim3(BLK), 0, st, sh, (const double *)d_pp, d_sc, d_d2);
    HIP_TRY(hipGetLastError());
    const dim3 g3((unsigned)((d + BLK - 1) / BLK), (unsigned)(L + (diff ? P : 0)));
    hipLaunchKernelGGL(k_field_fold_comp, g3, dim3(BLK), 0, st, sh, (const int32_t *)d_q, (const double *)d_pe, (const double *)d_pd,
                       d_se, d_d1);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sumse, d_se, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(sumsc, d_sc, mat, hipMemcpyDeviceToHost, st));
    if (diff) {
        if (P > 0) HIP_TRY(hipMemcpyAsync(sumsd1, d_d1, dvec, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(sumsd2, d_d2, mat, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

extern "C" int bluest_field_sums(int64_t S, int64_t d, const int64_t *counts, const int32_t *sizes, const double *const *values,
                                 const double *weights, int R, const int64_t *repeat_of, double *sums, double *mu, void *stream)
{
    if (S < 1) return fail(BLUEST_ERR_ARG, "S=%lld: at least one segment is needed", (long long)S);
    if (d < 1) return fail(BLUEST_ERR_ARG, "d=%lld: at least one component is needed", (long long)d);
    if (!counts || !sizes || !values || !sums) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((weights == nullptr) != (mu == nullptr)) return fail(BLUEST_ERR_ARG, "weights and mu must both be given or both be null");
    if (weights && (R < 1 || !repeat_of)) return fail(BLUEST_ERR_ARG, "with weights: R=%d >= 1 and repeat_of are needed", R);
    int64_t T = 0, nchunks = 0;
    double npart_f = 0.0;
    int Lmax = 1;
    for (int64_t s = 0; s < S; s++) {
        int rc = check_segment(s, counts, sizes, values, weights ? repeat_of : nullptr, R); if (rc) return rc;
        const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
        T += sizes[s];
        nchunks += nc;
        npart_f += (double)nc * sizes[s] * (double)d;
        Lmax = std::max(Lmax, (int)sizes[s]);
    }
    if (T > 0x7fffffffLL || nchunks > 0x7fffffffLL || (double)T * (double)d > 2147483647.0 || npart_f > 9.0e15)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 columns, column-components (T d) or chunks of %d samples in one call", GCHUNK);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;

    // ---- the tables: segments, the columns of every repeat ----
    std::vector<FSeg> segs((size_t)S);
    std::vector<int64_t> rep_cols(weights ? (size_t)R + 1 : 0, 0);
    std::vector<char> device((size_t)S), staged((size_t)S);
    std::vector<size_t> row_bytes((size_t)S);
    int64_t npart = 0;
    {
        int64_t col = 0;
        for (int64_t s = 0; s < S; s++) {
            const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK, W = sizes[s] * d;
            segs[s] = FSeg{npart, nc, W, col * d};
            col += sizes[s];
            npart += nc * W;
            if (weights) rep_cols[repeat_of[s] + 1] = col;              // repeat_of does not decrease: the last segment of a repeat wins
            device[s] = counts[s] > 0 && on_device(values[s]);
            staged[s] = counts[s] > 0 && !device[s];
            row_bytes[s] = (size_t)W * 8;
        }
        for (size_t r = 1; r < rep_cols.size(); r++) rep_cols[r] = std::max(rep_cols[r], rep_cols[r - 1]);   // a repeat without segments
    }
    const SlabPlan plan = plan_slabs(S, counts, row_bytes.data(), staged.data(), GCHUNK, (size_t)slab_budget());

    DeviceArena arena;
    const size_t vec = (size_t)T * d * 8;
    const size_t o_stage = arena.take(plan.stage_bytes + 256), o_part = arena.take((size_t)npart * 8),
                 o_chunks = arena.take((size_t)nchunks * sizeof(FChunk)), o_segs = arena.take((size_t)S * sizeof(FSeg)), o_sums = arena.take(vec),
                 o_w = arena.take(weights ? (size_t)T * 8 : 0), o_rc = arena.take(rep_cols.size() * 8),
                 o_mu = arena.take(weights ? (size_t)R * d * 8 : 0);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_stage = (const double *)(dv + o_stage);
    double *d_part = (double *)(dv + o_part), *d_sums = (double *)(dv + o_sums);
    FChunk *d_chunks = (FChunk *)(dv + o_chunks);

    // ---- the chunks: launch group 0 reads the device segments where they lie, group 1 + k the pieces of slab k ----
    ChunkLists<FChunk> chunks(1 + plan.slab_used.size(), 1, nchunks);
    auto add_chunks = [&](size_t g, int64_t s, const double *base, int64_t first, int64_t rows) {
        const int64_t W = segs[s].W;
        for (int64_t a = 0; a < rows; a += GCHUNK)
            chunks.add(g, 0, FChunk{base + a * W, segs[s].part + ((first + a) / GCHUNK) * W, W, (int32_t)std::min<int64_t>(GCHUNK, rows - a)});
    };
    for (int64_t s = 0; s < S; s++)
        if (device[s]) add_chunks(0, s, values[s], 0, counts[s]);
    for (const Piece &pc : plan.pieces) add_chunks(1 + (size_t)pc.slab, pc.seg, d_stage + pc.at / 8, pc.first, pc.rows);
    rc = chunks.flatten(); if (rc) return rc;
    if (nchunks > 0) HIP_TRY(hipMemcpyAsync(d_chunks, chunks.table.data(), (size_t)nchunks * sizeof(FChunk), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_segs, segs.data(), (size_t)S * sizeof(FSeg), hipMemcpyHostToDevice, st));

    const int64_t Wmax = (int64_t)Lmax * d;
    auto launch_group = [&](size_t g) -> hipError_t {
        const size_t c0 = chunks.begin(g), c1 = chunks.end(g);
        return bluest_partials::launch_fsum_partial(d_chunks + c0, c1 - c0, Wmax, d_part, st);
    };
    rc = run_slabs(plan, dv + o_stage, values, counts, row_bytes.data(), 1, launch_group, st); if (rc) return rc;
    const dim3 gf((unsigned)S, (unsigned)std::min<int64_t>((Wmax + FOLD_COLS - 1) / FOLD_COLS, 65535));
    hipLaunchKernelGGL(k_fsum_fold, gf, dim3(BLK), 0, st, (const FSeg *)(dv + o_segs), (const double *)d_part, d_sums);
    HIP_TRY(hipGetLastError());
    if (weights) {
        HIP_TRY(hipMemcpyAsync(dv + o_w, weights, (size_t)T * 8, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemcpyAsync(dv + o_rc, rep_cols.data(), rep_cols.size() * 8, hipMemcpyHostToDevice, st));
        const dim3 gm((unsigned)R, (unsigned)std::min<int64_t>((d + BLK - 1) / BLK, 65535));
        hipLaunchKernelGGL(k_fsum_mu, gm, dim3(BLK), 0, st, d, (const int64_t *)(dv + o_rc), (const double *)(dv + o_w),
                           (const double *)d_sums, (double *)(dv + o_mu));
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipMemcpyAsync(mu, dv + o_mu, (size_t)R * d * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipMemcpyAsync(sums, d_sums, vec, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

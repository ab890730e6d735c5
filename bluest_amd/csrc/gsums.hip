// gsums.hip -- Part 11 of include/bluest_hip.h: the sums over the samples of many model groups in one call, and the BLUE
// estimators those sums imply (what bluest/blue_fn.py:159-167 accumulates one Python addition per sample and model, and
// bluest/blue_models.py:555-571 / :963-968 repeat per group and per estimator of a variance test).
//
// Two launches per call (plus one k_gsum_partial per further slab of staged host data), no atomics, nothing sized by the device:
//   k_gsum_partial  grid (chunk, output) over a host-built table of chunks = (segment, first sample, rows <= BLUEST_GSUM_CHUNK):
//                   stages the chunk's rows x L values in LDS as they lie in memory, with 16-byte loads from the first 16-byte
//                   boundary on (at most one 8-byte load in front and one behind), then sums every column in the order the header
//                   states: eight classes of sixteen consecutive rows, each ascending, joined by a fixed tree.  The order is a
//                   property of the LDS image, so it cannot depend on the alignment of the source or on the width of a load.
//   k_gsum_fold     grid (fold group, output), fold group = one segment, or with weights all segments of one repeat: a wave per
//                   column, lane l adds the chunks l, l + 64, ... in ascending order, the lanes are joined by a fixed tree; with
//                   weights one thread then walks the group's columns in ascending order with fma.
// The segments' checks, the slabs of staged host data, the chunk table and the slab loop are those of staging.hpp.
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
static_assert((size_t)GCHUNK * BLUEST_MAX_MODELS * sizeof(double) <= 64 * 1024, "the staged chunk must fit the default LDS limit");
static_assert(CLASSES * BLUEST_MAX_MODELS <= 2 * BLK, "at most two (class, column) sums per thread");

std::atomic<int64_t> g_slab_bytes{BLUEST_GSUM_SLAB_BYTES};

struct GChunk {
    const double *src;      // row 0 of the chunk, output 0 (device address)
    int64_t ostride;        // doubles from output o to output o + 1 at `src`
    int64_t part;           // where the chunk's [n_out][L] partial sums start, in doubles
    int32_t rows, L;
};

struct GSeg {
    int64_t part;           // first chunk's partial sums
    int64_t nchunks;
    int32_t L, col0;
};

struct GFold {
    int64_t col0, col1;     // columns [col0, col1) of sums
    int64_t repeat;         // row of mu (with weights)
};

__global__ __launch_bounds__(BLK) void k_gsum_partial(const GChunk *__restrict__ table, double *__restrict__ part)
{
    extern __shared__ double tile[];
    const int tid = threadIdx.x;
    const GChunk d = table[blockIdx.x];
    const int64_t o = blockIdx.y;
    const int L = d.L, rows = d.rows, cnt = rows * L;
    const double *src = d.src + o * d.ostride;
    // src is 8-byte aligned: one value in front when it is not 16-byte aligned, pairs from there, one value behind when one is left
    const int head = (int)(((uintptr_t)src >> 3) & 1);
    const int npair = (cnt - head) >> 1;
    const double2 *pairs = (const double2 *)(src + head);
    for (int i = tid; i < npair; i += BLK) {
        const double2 v = pairs[i];
        tile[head + 2 * i] = v.x;
        tile[head + 2 * i + 1] = v.y;
    }
    if (tid == 0) {
        if (head) tile[0] = src[0];
        if ((cnt - head) & 1) tile[cnt - 1] = src[cnt - 1];
    }
    __syncthreads();

    double q[2];
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int p = tid + h * BLK;            // (class k, column j), column fastest: a wave reads consecutive LDS words
        q[h] = 0.0;
        if (p < CLASSES * L) {
            const int k = p / L, j = p - k * L;
            const int r1 = min((k + 1) * CLASS_ROWS, rows);
            for (int r = k * CLASS_ROWS; r < r1; r++) q[h] += tile[r * L + j];
        }
    }
    __syncthreads();                            // every read of the tile is done: the class sums go where it was
#pragma unroll
    for (int h = 0; h < 2; h++) {
        const int p = tid + h * BLK;
        if (p < CLASSES * L) tile[p] = q[h];
    }
    __syncthreads();
    if (tid < L) part[d.part + o * L + tid] = class_tree(tile + tid, L);
}

__global__ __launch_bounds__(BLK) void k_gsum_fold(const GFold *__restrict__ folds, const GSeg *__restrict__ segs,
                                                   const int32_t *__restrict__ col_seg, int n_out, int64_t T,
                                                   const double *__restrict__ part, const double *__restrict__ weights,
                                                   double *sums, double *__restrict__ mu)
{
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63;
    const GFold f = folds[blockIdx.x];
    const int64_t o = blockIdx.y;
    for (int64_t t = f.col0 + wave; t < f.col1; t += BLK / WAVE) {
        const GSeg s = segs[col_seg[t]];
        const double *src = part + s.part + o * s.L + (t - s.col0);
        const int64_t step = (int64_t)n_out * s.L;
        double acc = 0.0;
        for (int64_t c = lane; c < s.nchunks; c += WAVE) acc += src[c * step];
#pragma unroll
        for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, WAVE);      // lane l takes lane l + off: lane 0 ends with the tree
        if (lane == 0) sums[o * T + t] = acc;
    }
    if (weights == nullptr) return;
    __threadfence_block();
    __syncthreads();
    if (tid == 0) {
        double m = 0.0;
        for (int64_t t = f.col0; t < f.col1; t++) m = fma(weights[o * T + t], sums[o * T + t], m);
        mu[f.repeat * n_out + o] = m;
    }
}

}  // namespace

extern "C" int bluest_group_sums_slab(int64_t bytes, int64_t *previous)
{
    if (bytes < 0) return fail(BLUEST_ERR_ARG, "bytes=%lld: the staging budget cannot be negative (0 leaves it as it is)", (long long)bytes);
    if (previous) *previous = g_slab_bytes.load();
    if (bytes > 0) g_slab_bytes.store(bytes);
    return BLUEST_OK;
}

extern "C" int bluest_group_sums(int64_t S, int n_out, const int64_t *counts, const int32_t *sizes, const double *const *values,
                                 const double *weights, int R, const int64_t *repeat_of, double *sums, double *mu, void *stream)
{
    if (S < 1) return fail(BLUEST_ERR_ARG, "S=%lld: at least one segment is needed", (long long)S);
    if (n_out < 1 || n_out > BLUEST_GSUM_MAX_OUTPUTS)
        return fail(BLUEST_ERR_ARG, "n_out=%d out of range (1..%d)", n_out, BLUEST_GSUM_MAX_OUTPUTS);
    if (!counts || !sizes || !values || !sums) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((weights == nullptr) != (mu == nullptr)) return fail(BLUEST_ERR_ARG, "weights and mu must both be given or both be null");
    if (weights && (R < 1 || !repeat_of)) return fail(BLUEST_ERR_ARG, "with weights: R=%d >= 1 and repeat_of are needed", R);
    int64_t T = 0, nchunks = 0, npart = 0;
    int Lmax = 1;
    for (int64_t s = 0; s < S; s++) {
        int rc = check_segment(s, counts, sizes, values, weights ? repeat_of : nullptr, R); if (rc) return rc;
        const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
        T += sizes[s];
        nchunks += nc;
        npart += nc * n_out * sizes[s];
        Lmax = std::max(Lmax, (int)sizes[s]);
    }
    if (T > 0x7fffffffLL || nchunks > 0x7fffffffLL)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 columns or chunks of %d samples in one call", GCHUNK);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;

    // ---- the tables: segments, columns, fold groups ----
    std::vector<GSeg> segs((size_t)S);
    std::vector<int32_t> col_seg((size_t)T);
    std::vector<GFold> folds;
    std::vector<char> device((size_t)S), staged((size_t)S);
    std::vector<size_t> row_bytes((size_t)S);       // a row of a staged piece: [n_out][L]
    {
        int64_t col = 0, part = 0;
        for (int64_t s = 0; s < S; s++) {
            const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
            segs[s] = GSeg{part, nc, sizes[s], (int32_t)col};
            for (int j = 0; j < sizes[s]; j++) col_seg[col + j] = (int32_t)s;
            if (weights && !folds.empty() && folds.back().repeat == repeat_of[s]) folds.back().col1 = col + sizes[s];
            else folds.push_back(GFold{col, col + sizes[s], weights ? repeat_of[s] : 0});
            col += sizes[s];
            part += nc * n_out * sizes[s];
            device[s] = counts[s] > 0 && on_device(values[s]);
            staged[s] = counts[s] > 0 && !device[s];
            row_bytes[s] = (size_t)sizes[s] * 8 * n_out;
        }
    }
    const SlabPlan plan = plan_slabs(S, counts, row_bytes.data(), staged.data(), GCHUNK, (size_t)slab_budget());

    DeviceArena arena;
    const size_t vec = (size_t)n_out * T * 8;
    const size_t o_stage = arena.take(plan.stage_bytes + 256), o_part = arena.take((size_t)npart * 8),
                 o_chunks = arena.take((size_t)nchunks * sizeof(GChunk)), o_segs = arena.take((size_t)S * sizeof(GSeg)),
                 o_cols = arena.take((size_t)T * 4), o_folds = arena.take(folds.size() * sizeof(GFold)), o_sums = arena.take(vec),
                 o_w = arena.take(weights ? vec : 0), o_mu = arena.take(weights ? (size_t)R * n_out * 8 : 0);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_stage = (const double *)(dv + o_stage);
    double *d_part = (double *)(dv + o_part), *d_sums = (double *)(dv + o_sums);
    double *d_w = weights ? (double *)(dv + o_w) : nullptr, *d_mu = weights ? (double *)(dv + o_mu) : nullptr;
    GChunk *d_chunks = (GChunk *)(dv + o_chunks);

    // ---- the chunks: launch group 0 reads the device segments where they lie, group 1 + k the pieces of slab k ----
    ChunkLists<GChunk> chunks(1 + plan.slab_used.size(), 1, nchunks);
    auto add_chunks = [&](size_t g, int64_t s, const double *base, int64_t first, int64_t rows, int64_t ostride) {
        const int L = sizes[s];
        for (int64_t a = 0; a < rows; a += GCHUNK)
            chunks.add(g, 0, GChunk{base + a * L, ostride, segs[s].part + ((first + a) / GCHUNK) * n_out * L,
                                    (int32_t)std::min<int64_t>(GCHUNK, rows - a), L});
    };
    for (int64_t s = 0; s < S; s++)
        if (device[s]) add_chunks(0, s, values[s], 0, counts[s], counts[s] * sizes[s]);
    for (const Piece &pc : plan.pieces)
        add_chunks(1 + (size_t)pc.slab, pc.seg, d_stage + pc.at / 8, pc.first, pc.rows, pc.rows * sizes[pc.seg]);
    rc = chunks.flatten(); if (rc) return rc;
    if (nchunks > 0) HIP_TRY(hipMemcpyAsync(d_chunks, chunks.table.data(), (size_t)nchunks * sizeof(GChunk), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_segs, segs.data(), (size_t)S * sizeof(GSeg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_cols, col_seg.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_folds, folds.data(), folds.size() * sizeof(GFold), hipMemcpyHostToDevice, st));
    if (weights) {
        HIP_TRY(hipMemcpyAsync(d_w, weights, vec, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_mu, 0, (size_t)R * n_out * 8, st));
    }

    const size_t lds = (size_t)GCHUNK * Lmax * 8;
    auto launch_group = [&](size_t g) -> hipError_t {
        const size_t c0 = chunks.begin(g), c1 = chunks.end(g);
        if (c1 <= c0) return hipSuccess;
        hipLaunchKernelGGL(k_gsum_partial, dim3((unsigned)(c1 - c0), (unsigned)n_out), dim3(BLK), lds, st,
                           (const GChunk *)d_chunks + c0, d_part);
        return hipGetLastError();
    };
    rc = run_slabs(plan, dv + o_stage, values, counts, row_bytes.data(), n_out, launch_group, st); if (rc) return rc;
    hipLaunchKernelGGL(k_gsum_fold, dim3((unsigned)folds.size(), (unsigned)n_out), dim3(BLK), 0, st, (const GFold *)(dv + o_folds),
                       (const GSeg *)(dv + o_segs), (const int32_t *)(dv + o_cols), n_out, T, (const double *)d_part,
                       (const double *)d_w, d_sums, d_mu);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sums, d_sums, vec, hipMemcpyDeviceToHost, st));
    if (weights) HIP_TRY(hipMemcpyAsync(mu, d_mu, (size_t)R * n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

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
// Host segments are copied into one staging buffer slab by slab, every slab a whole number of chunks; the chunks' partial sums
// all land in one buffer that the single fold reads, so a slab boundary never shows in the result.
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
constexpr int CHUNK = BLUEST_GSUM_CHUNK;
constexpr int CLASSES = 8, CLASS_ROWS = CHUNK / CLASSES;
static_assert(CLASSES * CLASS_ROWS == CHUNK, "the row classes tile the chunk");
static_assert((size_t)CHUNK * BLUEST_MAX_MODELS * sizeof(double) <= 64 * 1024, "the staged chunk must fit the default LDS limit");
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
    if (tid < L) {
        const double *c = tile + tid;
        const double s = ((c[0] + c[L]) + (c[2 * L] + c[3 * L])) + ((c[4 * L] + c[5 * L]) + (c[6 * L] + c[7 * L]));
        part[d.part + o * L + tid] = s;
    }
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

struct Piece {              // rows [first, first + rows) of a host segment, staged as [n_out][rows][L] at `at` bytes of its slab
    int64_t seg, first, rows;
    size_t at;
    int slab;
};

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
        if (sizes[s] < 1 || sizes[s] > BLUEST_MAX_MODELS)
            return fail(BLUEST_ERR_ARG, "sizes[%lld]=%d out of range (1..%d)", (long long)s, sizes[s], BLUEST_MAX_MODELS);
        if (counts[s] < 0) return fail(BLUEST_ERR_ARG, "counts[%lld]=%lld is negative", (long long)s, (long long)counts[s]);
        if (counts[s] > 0 && !values[s]) return fail(BLUEST_ERR_ARG, "values[%lld] is null", (long long)s);
        if (counts[s] > 0 && ((uintptr_t)values[s] & 7)) return fail(BLUEST_ERR_ARG, "values[%lld] is not 8-byte aligned", (long long)s);
        if (weights) {
            if (repeat_of[s] < 0 || repeat_of[s] >= R)
                return fail(BLUEST_ERR_ARG, "repeat_of[%lld]=%lld out of range (0..%d)", (long long)s, (long long)repeat_of[s], R - 1);
            if (s > 0 && repeat_of[s] < repeat_of[s - 1]) return fail(BLUEST_ERR_ARG, "repeat_of decreases at segment %lld", (long long)s);
        }
        const int64_t nc = (counts[s] + CHUNK - 1) / CHUNK;
        T += sizes[s];
        nchunks += nc;
        npart += nc * n_out * sizes[s];
        Lmax = std::max(Lmax, (int)sizes[s]);
    }
    if (T > 0x7fffffffLL || nchunks > 0x7fffffffLL)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 columns or chunks of %d samples in one call", CHUNK);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;

    // ---- the tables: segments, columns, fold groups, chunks (device segments first, then the host pieces slab by slab) ----
    std::vector<GSeg> segs((size_t)S);
    std::vector<int32_t> col_seg((size_t)T);
    std::vector<GFold> folds;
    std::vector<GChunk> chunks;
    chunks.reserve((size_t)nchunks);
    std::vector<char> device((size_t)S);
    {
        int64_t col = 0, part = 0;
        for (int64_t s = 0; s < S; s++) {
            const int64_t nc = (counts[s] + CHUNK - 1) / CHUNK;
            segs[s] = GSeg{part, nc, sizes[s], (int32_t)col};
            for (int j = 0; j < sizes[s]; j++) col_seg[col + j] = (int32_t)s;
            if (weights && !folds.empty() && folds.back().repeat == repeat_of[s]) folds.back().col1 = col + sizes[s];
            else folds.push_back(GFold{col, col + sizes[s], weights ? repeat_of[s] : 0});
            col += sizes[s];
            part += nc * n_out * sizes[s];
            device[s] = counts[s] > 0 && on_device(values[s]);
        }
    }
    auto add_chunks = [&](int64_t s, const double *base, int64_t first, int64_t rows, int64_t ostride) {
        const int L = sizes[s];
        for (int64_t a = 0; a < rows; a += CHUNK)
            chunks.push_back(GChunk{base + a * L, ostride, segs[s].part + ((first + a) / CHUNK) * n_out * L,
                                    (int32_t)std::min<int64_t>(CHUNK, rows - a), L});
    };
    for (int64_t s = 0; s < S; s++)
        if (device[s]) add_chunks(s, values[s], 0, counts[s], counts[s] * sizes[s]);
    const size_t n_device_chunks = chunks.size();

    // slabs of the staging buffer: whole chunks only, each piece 256-byte aligned; a slab holds at least one chunk
    const size_t budget = std::max<size_t>((size_t)g_slab_bytes.load(), (size_t)CHUNK * Lmax * 8 * n_out + 256);
    std::vector<Piece> pieces;
    std::vector<size_t> slab_used;              // bytes per slab
    {
        size_t used = 0;
        int slab = 0;
        bool open = false;
        for (int64_t s = 0; s < S; s++) {
            if (device[s] || counts[s] == 0) continue;
            const size_t row_bytes = (size_t)sizes[s] * 8 * n_out;
            int64_t a = 0;
            while (a < counts[s]) {
                const int64_t rest = counts[s] - a;
                int64_t fit = (int64_t)((budget - used) / row_bytes);
                if (fit < rest) fit -= fit % CHUNK;
                if (fit <= 0) {                 // (an empty slab always fits a chunk: budget >= the widest chunk)
                    slab_used.push_back(used);
                    slab++;
                    used = 0;
                    continue;
                }
                const int64_t rows = std::min(rest, fit);
                pieces.push_back(Piece{s, a, rows, used, slab});
                used = std::min(budget, (used + (size_t)rows * row_bytes + 255) & ~(size_t)255);
                open = true;
                a += rows;
            }
        }
        if (open) slab_used.push_back(used);
    }
    const size_t stage_bytes = slab_used.empty() ? 0 : *std::max_element(slab_used.begin(), slab_used.end());

    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t vec = (size_t)n_out * T * 8;
    const size_t o_stage = take(stage_bytes + 256), o_part = take((size_t)npart * 8), o_chunks = take((size_t)nchunks * sizeof(GChunk)),
                 o_segs = take((size_t)S * sizeof(GSeg)), o_cols = take((size_t)T * 4), o_folds = take(folds.size() * sizeof(GFold)),
                 o_sums = take(vec), o_w = take(weights ? vec : 0), o_mu = take(weights ? (size_t)R * n_out * 8 : 0);
    char *dv = nullptr;
    HIP_TRY(hipMalloc(&dv, off));
    struct Free { char *p; ~Free() { if (p) (void)hipFree(p); } } guard{dv};
    const double *d_stage = (const double *)(dv + o_stage);
    double *d_part = (double *)(dv + o_part), *d_sums = (double *)(dv + o_sums);
    double *d_w = weights ? (double *)(dv + o_w) : nullptr, *d_mu = weights ? (double *)(dv + o_mu) : nullptr;
    GChunk *d_chunks = (GChunk *)(dv + o_chunks);

    // the chunk table of every slab is known before anything is copied: one upload
    std::vector<size_t> slab_chunk0;
    for (size_t p = 0; p < pieces.size(); p++) {
        if (p == 0 || pieces[p].slab != pieces[p - 1].slab) slab_chunk0.push_back(chunks.size());
        const Piece &pc = pieces[p];
        add_chunks(pc.seg, d_stage + pc.at / 8, pc.first, pc.rows, pc.rows * sizes[pc.seg]);
    }
    slab_chunk0.push_back(chunks.size());
    if ((int64_t)chunks.size() != nchunks) return fail(BLUEST_ERR_HIP, "internal: %zu chunks tabled, %lld expected", chunks.size(), (long long)nchunks);
    if (nchunks > 0) HIP_TRY(hipMemcpyAsync(d_chunks, chunks.data(), (size_t)nchunks * sizeof(GChunk), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_segs, segs.data(), (size_t)S * sizeof(GSeg), hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_cols, col_seg.data(), (size_t)T * 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(dv + o_folds, folds.data(), folds.size() * sizeof(GFold), hipMemcpyHostToDevice, st));
    if (weights) {
        HIP_TRY(hipMemcpyAsync(d_w, weights, vec, hipMemcpyHostToDevice, st));
        HIP_TRY(hipMemsetAsync(d_mu, 0, (size_t)R * n_out * 8, st));
    }

    const size_t lds = (size_t)CHUNK * Lmax * 8;
    auto launch_partial = [&](size_t c0, size_t c1) -> hipError_t {
        if (c1 <= c0) return hipSuccess;
        hipLaunchKernelGGL(k_gsum_partial, dim3((unsigned)(c1 - c0), (unsigned)n_out), dim3(BLK), lds, st,
                           (const GChunk *)d_chunks + c0, d_part);
        return hipGetLastError();
    };
    HIP_TRY(launch_partial(0, n_device_chunks));
    for (size_t p = 0, k = 0; p < pieces.size(); k++) {
        const int slab = pieces[p].slab;
        for (; p < pieces.size() && pieces[p].slab == slab; p++) {
            const Piece &pc = pieces[p];
            const int64_t L = sizes[pc.seg], N = counts[pc.seg];
            char *dst = dv + o_stage + pc.at;
            if (pc.rows == N) {
                HIP_TRY(hipMemcpyAsync(dst, values[pc.seg], (size_t)n_out * N * L * 8, hipMemcpyHostToDevice, st));
            } else {
                for (int o = 0; o < n_out; o++)
                    HIP_TRY(hipMemcpyAsync(dst + (size_t)o * pc.rows * L * 8, values[pc.seg] + ((int64_t)o * N + pc.first) * L,
                                           (size_t)pc.rows * L * 8, hipMemcpyHostToDevice, st));
            }
        }
        HIP_TRY(launch_partial(slab_chunk0[k], slab_chunk0[k + 1]));      // in stream order: the next slab's copies wait for it
    }
    hipLaunchKernelGGL(k_gsum_fold, dim3((unsigned)folds.size(), (unsigned)n_out), dim3(BLK), 0, st, (const GFold *)(dv + o_folds),
                       (const GSeg *)(dv + o_segs), (const int32_t *)(dv + o_cols), n_out, T, (const double *)d_part,
                       (const double *)d_w, d_sums, d_mu);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sums, d_sums, vec, hipMemcpyDeviceToHost, st));
    if (weights) HIP_TRY(hipMemcpyAsync(mu, d_mu, (size_t)R * n_out * 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

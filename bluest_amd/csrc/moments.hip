// moments.hip -- Part 13 of include/bluest_hip.h: first and second moments about the first sample of many ragged segments in one
// call (the sample covariance of every drawn model group: what gsums.hip adds up and throws away).
//
// The segments, the chunk table and the slabs of staged host data are those of staging.hpp, the fold is that of gsums.hip; what
// is its own is the work of a chunk.  Per call one k_mom_* launch per (slab, kernel shape) and one k_mom_fold, no atomics, nothing
// sized by the device:
//   k_mom_narrow / k_mom_wide  grid (chunk, output): stages the chunk's rows x L values in LDS as gsums.hip does (16-byte loads
//                   from the first 16-byte boundary on), SUBTRACTING THE SEGMENT'S FIRST SAMPLE on the way (one rounding per
//                   value), and fills the rows up to the next multiple of 16 with +0.0.  An ENTRY of a segment is one of its L
//                   columns (sum of d_j) or one of its L (L + 1) / 2 pairs (sum of d_j d_k), pairs numbered along the wrapped
//                   diagonals of staging.hpp.  Every entry is summed per class of sixteen consecutive rows, ascending
//                   (q += d resp. q = fma(d_j, d_k, q)), and the eight classes join in the fixed tree of Part 11.
//                   A row of +0.0 changes no bit: q starts at +0.0, and a sum that starts there is never -0.0.
//   k_mom_fold      grid (entries / 4, output): a wave per entry, lane l adds the chunks l, l + 64, ... in ascending order, the
//                   lanes join in the fixed tree; columns go to `first`, pairs to their place in the packed triangle of `second`.
// The shape follows L (moments_shape), because the chains of a chunk number 8 (L + L (L + 1) / 2):
//   L <= 4        k_mom_narrow<64>    one wavefront; a thread per (class, entry), at most 112 of them: two passes
//   5 <= L <= 22  k_mom_narrow<256>   a thread per (class, entry), at most 8 * 275 = 2200: nine passes; the class sums wait in
//                                     registers until every read of the tile is done, then go where the tile was (8 (L + P) <= 128 L)
//   L >= 23       k_mom_wide          a thread per entry (299 .. 2144 of them) with its eight class sums in registers
// Host segments are staged slab by slab (staging.hpp); the first-sample rows of all host segments travel in a buffer of
// their own, so a chunk in a later slab still finds its segment's shift.
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
constexpr int NARROW_1WAVE = 4, NARROW_MAX = 22;             // the widest L of k_mom_narrow<64> and of k_mom_narrow<256>
static_assert((size_t)GCHUNK * BLUEST_MAX_MODELS * sizeof(double) <= 64 * 1024, "the staged chunk must fit the default LDS limit");

__host__ __device__ constexpr int entries_of(int L) { return L + L * (L + 1) / 2; }
constexpr int passes_of(int L, int blk) { return (CLASSES * entries_of(L) + blk - 1) / blk; }
constexpr int NP_1WAVE = passes_of(NARROW_1WAVE, WAVE), NP_NARROW = passes_of(NARROW_MAX, BLK);
static_assert(CLASSES * entries_of(NARROW_MAX) <= GCHUNK * NARROW_MAX, "the class sums of a narrow chunk fit where its tile was");
static_assert(CLASSES * entries_of(NARROW_1WAVE) <= GCHUNK * NARROW_1WAVE && CLASSES * entries_of(1) <= GCHUNK, "and at every narrower L");

struct MChunk {
    const double *src;      // row 0 of the chunk, output 0 (device address)
    const double *shift;    // the segment's first sample, output 0 (device address): L values
    int64_t ostride;        // doubles from output o to output o + 1 at `src`
    int64_t sstride;        // ... at `shift`
    int64_t part;           // where the chunk's [n_out][L + P] partial sums start, in doubles
    int32_t rows, L;
};

struct MSeg {
    int64_t part;           // first chunk's partial sums
    int64_t nchunks;
    int64_t ent0;           // the segment's first entry
    int64_t col0, pair0;    // its first column of `first` and its first packed pair of `second`
    int32_t L;
};

// the chunk as d = value - shift, rows [rows, ceil16(rows)) = +0.0
template <int B>
__device__ __forceinline__ void stage_shifted(double *tile, const MChunk &d, int64_t o, int tid)
{
    const int L = d.L, cnt = d.rows * L, padded = ((d.rows + CLASS_ROWS - 1) & ~(CLASS_ROWS - 1)) * L;
    const double *src = d.src + o * d.ostride;
    const double *sh = d.shift + o * d.sstride;
    // src is 8-byte aligned: one value in front when it is not 16-byte aligned, pairs from there, one value behind when one is left
    const int head = (int)(((uintptr_t)src >> 3) & 1);
    const int npair = (cnt - head) >> 1;
    const double2 *pairs = (const double2 *)(src + head);
    const int step = (2 * B) % L;
    int j = (head + 2 * tid) % L;                               // the column of element head + 2 i
    for (int i = tid; i < npair; i += B) {
        const double2 v = pairs[i];
        const int j1 = j + 1 == L ? 0 : j + 1;
        tile[head + 2 * i] = v.x - sh[j];
        tile[head + 2 * i + 1] = v.y - sh[j1];
        j += step;
        if (j >= L) j -= L;
    }
    if (tid == 0) {
        if (head) tile[0] = src[0] - sh[0];
        if ((cnt - head) & 1) tile[cnt - 1] = src[cnt - 1] - sh[L - 1];
    }
    for (int t = cnt + tid; t < padded; t += B) tile[t] = 0.0;
}

// one class of one entry: sixteen rows from `base` on, ascending
__device__ __forceinline__ double class_sum(const double *base, int L, int e)
{
    double q = 0.0;
    if (e < L) {
#pragma unroll
        for (int r = 0; r < CLASS_ROWS; r++) q += base[r * L + e];
    } else {
        int lo, hi;
        pair_of(e - L, L, lo, hi);
#pragma unroll
        for (int r = 0; r < CLASS_ROWS; r++) q = fma(base[r * L + lo], base[r * L + hi], q);
    }
    return q;
}

template <int B, int NP>
__global__ __launch_bounds__(B) void k_mom_narrow(const MChunk *__restrict__ table, double *__restrict__ part)
{
    extern __shared__ double tile[];
    const int tid = threadIdx.x;
    const MChunk d = table[blockIdx.x];
    const int64_t o = blockIdx.y;
    const int L = d.L, W = entries_of(L), items = CLASSES * W;
    stage_shifted<B>(tile, d, o, tid);
    __syncthreads();

    double q[NP];
#pragma unroll
    for (int h = 0; h < NP; h++) {
        const int p = tid + h * B;                  // (class k, entry e), entry fastest: a half-wave reads one row
        q[h] = 0.0;
        if (p < items) {
            const int k = p / W, e = p - k * W;
            if (k * CLASS_ROWS < d.rows) q[h] = class_sum(tile + k * CLASS_ROWS * L, L, e);
        }
    }
    __syncthreads();                                // every read of the tile is done: the class sums go where it was
#pragma unroll
    for (int h = 0; h < NP; h++) {
        const int p = tid + h * B;
        if (p < items) tile[p] = q[h];
    }
    __syncthreads();
    for (int e = tid; e < W; e += B) part[d.part + o * W + e] = class_tree(tile + e, W);
}

__global__ __launch_bounds__(BLK) void k_mom_wide(const MChunk *__restrict__ table, double *__restrict__ part)
{
    extern __shared__ double tile[];
    const int tid = threadIdx.x;
    const MChunk d = table[blockIdx.x];
    const int64_t o = blockIdx.y;
    const int L = d.L, W = entries_of(L);
    const int kcount = (d.rows + CLASS_ROWS - 1) / CLASS_ROWS;
    stage_shifted<BLK>(tile, d, o, tid);
    __syncthreads();
    for (int e = tid; e < W; e += BLK) {
        double q[CLASSES];
#pragma unroll
        for (int k = 0; k < CLASSES; k++) {
            q[k] = 0.0;
            if (k < kcount) q[k] = class_sum(tile + k * CLASS_ROWS * L, L, e);
        }
        part[d.part + o * W + e] = class_tree(q);
    }
}

__global__ __launch_bounds__(BLK) void k_mom_fold(const MSeg *__restrict__ segs, const int32_t *__restrict__ ent_seg, int64_t E,
                                                  int n_out, int64_t T, int64_t P, const double *__restrict__ part,
                                                  double *__restrict__ first, double *__restrict__ second)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (BLK / WAVE) + (threadIdx.x >> 6), o = blockIdx.y;
    if (e >= E) return;                             // (a whole wave leaves: the shuffles below see all of their lanes)
    const MSeg s = segs[ent_seg[e]];
    const int L = s.L, W = entries_of(L), idx = (int)(e - s.ent0);
    const double *src = part + s.part + o * W + idx;
    const int64_t step = (int64_t)n_out * W;
    double acc = 0.0;
    for (int64_t c = lane; c < s.nchunks; c += WAVE) acc += src[c * step];
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, WAVE);      // lane l takes lane l + off: lane 0 ends with the tree
    if (lane != 0) return;
    if (idx < L) first[o * T + s.col0 + idx] = acc;
    else {
        int lo, hi;
        pair_of(idx - L, L, lo, hi);
        second[o * P + s.pair0 + lo * L - lo * (lo - 1) / 2 + (hi - lo)] = acc;
    }
}

enum { SHAPE_1WAVE = 0, SHAPE_NARROW = 1, SHAPE_WIDE = 2, SHAPES = 3 };
int moments_shape(int L) { return L <= NARROW_1WAVE ? SHAPE_1WAVE : L <= NARROW_MAX ? SHAPE_NARROW : SHAPE_WIDE; }

}  // namespace

extern "C" int bluest_group_moments(int64_t S, int n_out, const int64_t *counts, const int32_t *sizes, const double *const *values,
                                    double *first, double *second, void *stream)
{
    if (S < 1) return fail(BLUEST_ERR_ARG, "S=%lld: at least one segment is needed", (long long)S);
    if (n_out < 1 || n_out > BLUEST_GSUM_MAX_OUTPUTS)
        return fail(BLUEST_ERR_ARG, "n_out=%d out of range (1..%d)", n_out, BLUEST_GSUM_MAX_OUTPUTS);
    if (!counts || !sizes || !values || !first || !second) return fail(BLUEST_ERR_ARG, "null pointer");
    int64_t T = 0, P = 0, nchunks = 0, npart = 0;
    int Lmax[SHAPES] = {0, 0, 0};
    for (int64_t s = 0; s < S; s++) {
        int rc = check_segment(s, counts, sizes, values); if (rc) return rc;
        const int L = sizes[s];
        const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
        T += L;
        P += L * (L + 1) / 2;
        nchunks += nc;
        npart += nc * n_out * entries_of(L);
        Lmax[moments_shape(L)] = std::max(Lmax[moments_shape(L)], L);
    }
    if (T > 0x7fffffffLL || nchunks > 0x7fffffffLL)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 columns or chunks of %d samples in one call", GCHUNK);
    if (P > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 packed pairs in one call");
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    const int64_t E = T + P;

    // ---- the tables: segments, entries ----
    std::vector<MSeg> segs((size_t)S);
    std::vector<int32_t> ent_seg((size_t)E);
    std::vector<char> device((size_t)S), staged((size_t)S);
    std::vector<size_t> row_bytes((size_t)S);          // a row of a staged piece: [n_out][L]
    std::vector<int64_t> shift_at((size_t)S, -1);      // host segments: where the first-sample rows [n_out][L] lie in the shift buffer
    int64_t nshift = 0;
    {
        int64_t col = 0, pair = 0, part = 0, ent = 0;
        for (int64_t s = 0; s < S; s++) {
            const int L = sizes[s];
            const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
            segs[s] = MSeg{part, nc, ent, col, pair, L};
            std::fill(ent_seg.begin() + ent, ent_seg.begin() + ent + entries_of(L), (int32_t)s);
            col += L;
            pair += L * (L + 1) / 2;
            ent += entries_of(L);
            part += nc * n_out * entries_of(L);
            device[s] = counts[s] > 0 && on_device(values[s]);
            staged[s] = counts[s] > 0 && !device[s];
            row_bytes[s] = (size_t)L * 8 * n_out;
            if (staged[s]) {
                shift_at[s] = nshift;
                nshift += (int64_t)n_out * L;
            }
        }
    }
    std::vector<double> shifts((size_t)nshift);
    for (int64_t s = 0; s < S; s++)
        if (shift_at[s] >= 0)
            for (int o = 0; o < n_out; o++)
                std::memcpy(shifts.data() + shift_at[s] + (int64_t)o * sizes[s], values[s] + (int64_t)o * counts[s] * sizes[s],
                            (size_t)sizes[s] * 8);

    const SlabPlan plan = plan_slabs(S, counts, row_bytes.data(), staged.data(), GCHUNK, (size_t)slab_budget());

    DeviceArena arena;
    const size_t b_first = (size_t)n_out * T * 8, b_second = (size_t)n_out * P * 8;
    const size_t o_stage = arena.take(plan.stage_bytes + 256), o_shift = arena.take((size_t)nshift * 8), o_part = arena.take((size_t)npart * 8),
                 o_chunks = arena.take((size_t)nchunks * sizeof(MChunk)), o_segs = arena.take((size_t)S * sizeof(MSeg)),
                 o_ents = arena.take((size_t)E * 4), o_first = arena.take(b_first), o_second = arena.take(b_second);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_stage = (const double *)(dv + o_stage), *d_shift = (const double *)(dv + o_shift);
    double *d_part = (double *)(dv + o_part), *d_first = (double *)(dv + o_first), *d_second = (double *)(dv + o_second);
    MChunk *d_chunks = (MChunk *)(dv + o_chunks);

    // ---- the chunks: launch group 0 reads the device segments where they lie, group 1 + k the pieces of slab k; a list per shape ----
    ChunkLists<MChunk> chunks(1 + plan.slab_used.size(), SHAPES, nchunks);
    auto add_chunks = [&](size_t g, int64_t s, const double *base, int64_t first_row, int64_t rows, int64_t ostride,
                          const double *shift, int64_t sstride) {
        const int L = sizes[s], W = entries_of(L);
        for (int64_t a = 0; a < rows; a += GCHUNK)
            chunks.add(g, moments_shape(L), MChunk{base + a * L, shift, ostride, sstride, segs[s].part + ((first_row + a) / GCHUNK) * n_out * W,
                                                   (int32_t)std::min<int64_t>(GCHUNK, rows - a), L});
    };
    for (int64_t s = 0; s < S; s++)
        if (device[s]) add_chunks(0, s, values[s], 0, counts[s], counts[s] * sizes[s], values[s], counts[s] * sizes[s]);
    for (const Piece &pc : plan.pieces)
        add_chunks(1 + (size_t)pc.slab, pc.seg, d_stage + pc.at / 8, pc.first, pc.rows, pc.rows * sizes[pc.seg],
                   d_shift + shift_at[pc.seg], sizes[pc.seg]);
    rc = chunks.flatten(); if (rc) return rc;
    // the tables lie side by side on the device: one image of them on the host, one copy
    std::vector<char> tables(o_first - o_chunks);
    if (nchunks > 0) std::memcpy(tables.data(), chunks.table.data(), (size_t)nchunks * sizeof(MChunk));
    std::memcpy(tables.data() + (o_segs - o_chunks), segs.data(), (size_t)S * sizeof(MSeg));
    std::memcpy(tables.data() + (o_ents - o_chunks), ent_seg.data(), (size_t)E * 4);
    HIP_TRY(hipMemcpyAsync(dv + o_chunks, tables.data(), tables.size(), hipMemcpyHostToDevice, st));
    if (nshift > 0) HIP_TRY(hipMemcpyAsync(dv + o_shift, shifts.data(), (size_t)nshift * 8, hipMemcpyHostToDevice, st));

    auto launch_group = [&](size_t g) -> hipError_t {
        for (int shape = 0; shape < SHAPES; shape++) {
            const size_t c0 = chunks.begin(g, shape), c1 = chunks.end(g, shape);
            if (c1 <= c0) continue;
            const dim3 grid((unsigned)(c1 - c0), (unsigned)n_out);
            const size_t lds = (size_t)GCHUNK * Lmax[shape] * 8;
            const MChunk *table = d_chunks + c0;
            if (shape == SHAPE_1WAVE) hipLaunchKernelGGL((k_mom_narrow<WAVE, NP_1WAVE>), grid, dim3(WAVE), lds, st, table, d_part);
            else if (shape == SHAPE_NARROW) hipLaunchKernelGGL((k_mom_narrow<BLK, NP_NARROW>), grid, dim3(BLK), lds, st, table, d_part);
            else hipLaunchKernelGGL(k_mom_wide, grid, dim3(BLK), lds, st, table, d_part);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    rc = run_slabs(plan, dv + o_stage, values, counts, row_bytes.data(), n_out, launch_group, st); if (rc) return rc;
    hipLaunchKernelGGL(k_mom_fold, dim3((unsigned)((E + BLK / WAVE - 1) / (BLK / WAVE)), (unsigned)n_out), dim3(BLK), 0, st,
                       (const MSeg *)(dv + o_segs), (const int32_t *)(dv + o_ents), E, n_out, T, P, (const double *)d_part, d_first,
                       d_second);
    HIP_TRY(hipGetLastError());
    std::vector<char> results(o_second - o_first + b_second);            // `first` and `second` lie side by side too: one copy back
    HIP_TRY(hipMemcpyAsync(results.data(), d_first, results.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(first, results.data(), b_first);
    std::memcpy(second, results.data() + (o_second - o_first), b_second);
    return BLUEST_OK;
}

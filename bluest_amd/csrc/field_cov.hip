// field_cov.hip -- Part 16 of include/bluest_hip.h: per ragged segment of counts[s] x sizes[s] x d field values the second moments
// about the first sample of every pair of models in the inner product <a, b> = sum_c w_c a_c b_c (`second`), the inner products
// of the first moments (`cross`, formed on the device) and, on request, the first moments themselves (`first`): what the
// unbiased covariance of every drawn model group of a field output is made of, (second - cross / N) / (N - 1).
//
// The segments, the chunk table, the slabs of staged host data and the slab loop are those of staging.hpp; the first-sample rows
// of the host segments travel in a buffer of their own, as in moments.hip, so a chunk in a later slab still finds its segment's
// shift.  What is its own is the work of a chunk.  Per call one k_fcov_partial launch per (slab, TB) and three folds; no atomics,
// nothing sized by the device, no matrix instructions.
//   k_fcov_partial      1-D grid over (chunk of the table, block of TB component tiles), 256 threads.  The block's part of the
//                       shift row, [L][8 TB], is staged in LDS once.  The chunk is then walked in SUB-BLOCKS of sb samples:
//                       sb x L x 8 TB values are read from memory in runs along c, the fastest index, shifted on the way (one
//                       rounding per value) and laid out as fields.hip does, [tile of the block][sample][model][8 components +
//                       1 pad]: the odd stride of 9 doubles keeps 32 consecutive models on 32 different bank pairs for a 64-bit
//                       LDS read.  BLK / TB consecutive threads share a tile; thread j of them owns the pairs j, j + BLK / TB, ...
//                       of that tile, pairs numbered along the wrapped diagonals of staging.hpp, and walks s ascending, then c
//                       ascending inside the tile: q = fma(w_c * a, b, q).  A thread per (model, component) of the block adds
//                       q += d for f; its class sums go to memory as they are (1 / 16 of what the chunk reads), and
//                       k_fcov_fold_first joins them in the tree, as the split form of field_moments.hip does.  sb divides the sixteen samples of a class, so a class ends where a sub-block ends; there
//                       the class sum q joins the pending sums of the fixed tree ((q0+q1)+(q2+q3))+((q4+q5)+(q6+q7)) and starts
//                       again from +0.0.  The tree is evaluated as the classes arrive: three pending sums per chain (an even
//                       class, a pair of classes, the first four classes), not eight accumulators.  A class without samples joins as +0.0.
//                       Output: partp [pair][chunk of the segment][tile] and partf [chunk of the segment][class][model][component].
//   k_fcov_fold_second  a wave per (segment, pair): per chunk, lane l adds the tiles l, l + 64, ... in ascending order and the
//                       lanes join in the butterfly, whose lane 0 is the tree of Part 11 and which leaves the same bits in every
//                       lane; lane c mod 64 then takes the value of chunk c, so lane l adds the chunks l, l + 64, ... in
//                       ascending order, and the lanes join in the tree of Part 11, step 3.
//   k_fcov_fold_first   grid (segment, block of 64 column-components), as k_fsum_fold of fields.hip: wave g = 0..3 computes the
//                       lane sums l = g, g + 4, ... of Part 11 step 3 into LDS, coalesced along c, a chunk's value being the
//                       tree over its eight class sums; then the tree of the lanes runs over LDS.
//                       The result f stays in a device buffer [T][d].
//   k_fcov_cross        a wave per (segment, pair): lane l walks the tiles l, l + 64, ...: x = fma(w_c * f_j[c], f_k[c], x) over
//                       the tile's components from +0.0, the tiles' values added in ascending order from +0.0; the tree joins the
//                       lanes.  f is copied to the host only where `first` is given.
//
// THE LAUNCH SHAPE (field_cov_tiles, field_cov_rows; decided on the host per segment, carried by the chunk table; it never enters
// the order of an operation: a pair's chain of a (chunk, tile, class) is one thread's whatever TB and sb are):
//   TB  tiles per workgroup: the largest power of two <= 16 with n_pairs(L) TB <= KMAX BLK = 2304 and 8 L TB <= EMAX BLK = 2048,
//       and no more than it takes to cover the ceil(d / 8) tiles there are.  Where d >= 128: L <= 16: 16, L <= 23: 8, L <= 33: 4,
//       L <= 47: 2, else 1.  A narrow group has few pairs, so a workgroup takes several tiles side by side, which also
//       makes the runs along c longer (1 KB per model and sample at TB = 16).
//   sb  samples per sub-block: the largest power of two <= 16 with sb TB L 72 bytes <= 40 KB of LDS (at L = 64: 8 samples in
//       36 KB), at least 1.  With the shift row (L TB 64 bytes, at most 16 KB) a workgroup stays below 56 KB: two workgroups per
//       compute unit, which is what its registers allow anyway.
//   The classes of a chunk are NOT spread over threads for narrow groups: at L = 1 one thread in sixteen owns a pair.  Such a
//   group moves few bytes per pair, all 256 threads stage, and the walk of a sub-block (sb x 8 fma per pair) hides behind the
//   staging of the next workgroup on the same compute unit.
// KMAX = 9 pairs per thread, four doubles each (q and three pending sums), and EMAX = 8 first-moment chains of one double are 88
// VGPRs of sums; the LDS offsets of a pair share one register (DESIGN section 16 has the resource table: no scratch).
#include "staging.hpp"

namespace {

constexpr int BLK = 256;
constexpr int TILE = BLUEST_FIELD_TILE;
constexpr int STR = TILE + 1;                       // doubles from model i to model i + 1 in LDS
constexpr int KMAX = (BLUEST_MAX_MODELS * (BLUEST_MAX_MODELS + 1) / 2 + BLK - 1) / BLK;     // pairs per thread: 9
constexpr int EMAX = 8;                             // (model, component) chains per thread: L * TILE * TB <= EMAX * BLK
constexpr int TB_MAX = 16, TB_KEYS = 5;             // TB = 1 << key
constexpr size_t TILE_BYTES = 40 * 1024;            // LDS of the staged sub-block
constexpr int FOLD_COLS = 64;
static_assert(TILE == 8, "the shifts and masks below take a tile of 8 components");
static_assert((size_t)BLUEST_MAX_MODELS * STR * 8 <= TILE_BYTES, "one sample of the widest group fits the sub-block");
static_assert(TILE_BYTES + (size_t)EMAX * BLK * 8 <= 64 * 1024, "sub-block and shift row fit the default LDS");

int field_cov_tiles(int L, int64_t ntiles)
{
    int tb = 1;
    while (tb < TB_MAX && tb < ntiles && n_pairs(L) * 2 * tb <= KMAX * BLK && L * TILE * 2 * tb <= EMAX * BLK) tb *= 2;
    return tb;
}

int field_cov_rows(int L, int tb)
{
    int sb = CLASS_ROWS;
    while (sb > 1 && (size_t)sb * tb * L * STR * 8 > TILE_BYTES) sb >>= 1;
    return sb;
}

struct CChunk {
    const double *src;      // row 0 of the chunk (device address)
    const double *shift;    // the segment's first sample (device address): L d values
    int64_t partp;          // the chunk's partial sums of pair 0, tile 0, in doubles
    int64_t pstride;        // doubles from pair q to pair q + 1: (chunks of the segment) * ntiles
    int64_t partf;          // the chunk's [class][L][d] class sums of d
    int32_t rows, L;
    int32_t sb, pad;
};

struct CSeg {
    int64_t partp, partf;   // first chunk's partial sums
    int64_t nchunks;
    int64_t pair0, col0;    // the segment's first packed pair and first column
    int32_t L, pad;
};

// Class k of the thread's chains is complete with the sums q: the tree ((q0+q1)+(q2+q3))+((q4+q5)+(q6+q7)) as far as it can be
// formed, and q starts again from +0.0.  Three pending sums per chain: a1 an even class, a2 a pair, a3 the first four classes.  k
// is uniform over the workgroup.  After k = 7, a3 holds the chunk's values.
__device__ __forceinline__ void tree_step(int k, double (&q)[KMAX], double (&a1)[KMAX], double (&a2)[KMAX], double (&a3)[KMAX])
{
#pragma unroll
    for (int i = 0; i < KMAX; i++) {
        const double x = q[i];
        q[i] = 0.0;
        if ((k & 1) == 0) { a1[i] = x; continue; }
        const double pair = a1[i] + x;
        if ((k & 2) == 0) { a2[i] = pair; continue; }
        const double quad = a2[i] + pair;
        a3[i] = (k & 4) == 0 ? quad : a3[i] + quad;
    }
}

template <bool FULL>
__device__ __forceinline__ void fcov_partial_body(const CChunk &ch, int64_t d, int64_t ntiles, int64_t blk, int tb_shift,
                                                  const double *__restrict__ w, double *__restrict__ partp, double *__restrict__ partf,
                                                  double *lds)
{
    const int tid = threadIdx.x;
    const int L = ch.L, TB = 1 << tb_shift, sb = ch.sb;
    const int64_t cb0 = blk * TB * TILE;                               // first component of the block
    const int bw = (int)min((int64_t)TB * TILE, d - cb0);              // components of the block
    const int bwp = TB * TILE, bshift = tb_shift + 3;                  // padded width, a power of two
    double *shl = lds, *tile = lds + L * bwp;                          // the shift row [L][bwp]; the sub-block
    // the thread's tile and pairs: BLK / TB consecutive threads share a tile, thread j of them owns the pairs j, j + BLK / TB, ...
    const int npairs = n_pairs(L), G = BLK >> tb_shift, tb = tid >> (8 - tb_shift), pl = tid & (G - 1);
    const int kcount = (npairs + G - 1) / G;
    const int tw = FULL ? TILE : max(0, min(TILE, bw - tb * TILE));    // components of the thread's tile
    const int at_tile = tb * sb * L * STR;

    for (int t = tid; t < (L << bshift); t += BLK) {
        const int c = t & (bwp - 1);
        if (FULL || c < bw) shl[t] = ch.shift[(int64_t)(t >> bshift) * d + cb0 + c];
    }

    int at_pair[KMAX];                                                 // LDS offsets of the pair's two models, 16 bits each
    double q[KMAX], s0[KMAX], s1[KMAX], s2[KMAX], wc[TILE];
#pragma unroll
    for (int c = 0; c < TILE; c++) wc[c] = c < tw ? w[cb0 + tb * TILE + c] : 0.0;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int pr = pl + k * G;
        int lo = 0, hi = 0;
        if (pr < npairs) pair_of(pr, L, lo, hi);
        at_pair[k] = (at_tile + lo * STR) | ((at_tile + hi * STR) << 16);
        q[k] = s0[k] = s1[k] = s2[k] = 0.0;
    }
    // the thread's chains of f: (model i_e + m e_step, component c_e of the block), m = 0..EMAX-1, where that model exists
    const int c_e = tid & (bwp - 1), i_e = tid >> bshift, e_step = BLK >> bshift;
    const int at_e = ((c_e >> 3) * sb * L + i_e) * STR + (c_e & 7);
    const int e_count = c_e < bw ? min(EMAX, (L - i_e + e_step - 1) / e_step) : 0;      // (negative where i_e >= L)
    const int64_t W = (int64_t)L * d;
    double *dst_e = partf + ch.partf + (int64_t)i_e * d + cb0 + c_e;
    double e[EMAX];
#pragma unroll
    for (int m = 0; m < EMAX; m++) e[m] = 0.0;
    const float inv_L = 1.0f / (float)L;

    for (int sub = 0; sub < ch.rows; sub += sb) {
        const int nsb = min(sb, ch.rows - sub), rows = nsb * L;
        __syncthreads();                                               // every read of the last sub-block is done (first pass: the shift row is there)
        const double *src = ch.src + (int64_t)sub * L * d + cb0;
#pragma unroll 4
        for (int t = tid; t < (rows << bshift); t += BLK) {            // runs of bw components along c, the fastest index
            const int row = t >> bshift, c = t & (bwp - 1);
            const int s = (int)(((float)row + 0.5f) * inv_L), i = row - s * L;      // row = s L + i, exact: row < 1024, L <= 64
            if (FULL || c < bw) tile[((c >> 3) * sb * L + row) * STR + (c & 7)] = src[(int64_t)row * d + c] - shl[(i << bshift) + c];
        }
        __syncthreads();
        for (int s = 0; s < nsb; s++) {
            const double *row = tile + s * L * STR;
#pragma unroll
            for (int m = 0; m < EMAX; m++)
                if (m < e_count) e[m] += row[at_e + m * e_step * STR];
#pragma unroll
            for (int k = 0; k < KMAX; k++) {
                if (k < kcount) {
                    const double *ya = row + (at_pair[k] & 0xffff), *yb = row + (at_pair[k] >> 16);
#pragma unroll
                    for (int c = 0; c < TILE; c++)
                        if (FULL || c < tw) q[k] = fma(wc[c] * ya[c], yb[c], q[k]);
                }
            }
        }
        const int done = sub + nsb;
        if ((done & (CLASS_ROWS - 1)) == 0 || done == ch.rows) {       // the class is complete
            const int cls = (done - 1) / CLASS_ROWS;
            tree_step(cls, q, s0, s1, s2);
#pragma unroll
            for (int m = 0; m < EMAX; m++) {
                if (m < e_count) dst_e[cls * W + (int64_t)m * e_step * d] = e[m];
                e[m] = 0.0;
            }
        }
    }
    for (int cls = (ch.rows + CLASS_ROWS - 1) / CLASS_ROWS; cls < CLASSES; cls++) {     // the classes without samples: +0.0
        tree_step(cls, q, s0, s1, s2);                                  // (q is +0.0 again)
#pragma unroll
        for (int m = 0; m < EMAX; m++)
            if (m < e_count) dst_e[cls * W + (int64_t)m * e_step * d] = 0.0;
    }

    const int64_t t = blk * TB + tb;
#pragma unroll
    for (int k = 0; k < KMAX; k++) {
        const int pr = pl + k * G;
        if (pr < npairs && tw > 0 && t < ntiles) partp[ch.partp + (int64_t)pr * ch.pstride + t] = s2[k];
    }
}

// grid: (chunks of the launch) * nblocks, nblocks = ceil(ntiles / TB)
__global__ __launch_bounds__(BLK) void k_fcov_partial(const CChunk *__restrict__ table, int64_t d, int64_t ntiles, int64_t nblocks,
                                                      int tb_shift, const double *__restrict__ w, double *__restrict__ partp,
                                                      double *__restrict__ partf)
{
    extern __shared__ double lds[];
    const int64_t b = blockIdx.x, local = b / nblocks, blk = b - local * nblocks;
    const CChunk ch = table[local];
    if ((blk + 1) * ((int64_t)TILE << tb_shift) <= d) fcov_partial_body<true>(ch, d, ntiles, blk, tb_shift, w, partp, partf, lds);
    else fcov_partial_body<false>(ch, d, ntiles, blk, tb_shift, w, partp, partf, lds);
}

// a wave per packed pair of the call; ent_seg[e]: its segment
__global__ __launch_bounds__(BLK) void k_fcov_fold_second(const CSeg *__restrict__ segs, const int32_t *__restrict__ ent_seg, int64_t P,
                                                          int64_t ntiles, const double *__restrict__ partp, double *__restrict__ second)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (BLK / WAVE) + (threadIdx.x >> 6);
    if (e >= P) return;                                                // whole waves leave
    const CSeg s = segs[ent_seg[e]];
    const int L = s.L, pr = (int)(e - s.pair0);
    const double *src = partp + s.partp + (int64_t)pr * s.nchunks * ntiles;
    double p = 0.0;
    for (int64_t c = 0; c < s.nchunks; c++) {
        double acc = 0.0;
        for (int64_t t = lane; t < ntiles; t += WAVE) acc += src[c * ntiles + t];
        const double v = wave_sum(acc);                                // lane 0's tree; every lane ends with the same bits
        if ((c & 63) == lane) p += v;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) p += __shfl_down(p, off, WAVE);         // lane l takes lane l + off: lane 0 ends with the tree
    if (lane != 0) return;
    int lo, hi;
    pair_of(pr, L, lo, hi);
    second[s.pair0 + lo * L - lo * (lo - 1) / 2 + (hi - lo)] = p;
}

// grid (segment, block of 64 column-components)
__global__ __launch_bounds__(BLK) void k_fcov_fold_first(const CSeg *__restrict__ segs, int64_t d, const double *__restrict__ partf,
                                                         double *__restrict__ f)
{
    __shared__ double p[WAVE][FOLD_COLS];
    const CSeg sg = segs[blockIdx.x];
    const int tid = threadIdx.x, g = tid >> 6, j = tid & 63;
    const int64_t W = sg.L * d;
    for (int64_t col0 = (int64_t)blockIdx.y * FOLD_COLS; col0 < W; col0 += (int64_t)gridDim.y * FOLD_COLS) {
        const int64_t col = col0 + j;
        for (int l = g; l < WAVE; l += BLK / WAVE) {
            double acc = 0.0;
            if (col < W)
                for (int64_t c = l; c < sg.nchunks; c += WAVE) {        // the chunk's eight class sums join in the tree
                    const double *q = partf + sg.partf + c * CLASSES * W + col;
                    acc += ((q[0] + q[W]) + (q[2 * W] + q[3 * W])) + ((q[4 * W] + q[5 * W]) + (q[6 * W] + q[7 * W]));
                }
            p[l][j] = acc;
        }
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) {                       // lane l < off takes p_l + p_(l + off)
            for (int v = tid; v < off * FOLD_COLS; v += BLK) p[v >> 6][v & 63] += p[(v >> 6) + off][v & 63];
            __syncthreads();
        }
        if (tid < FOLD_COLS && col < W) f[sg.col0 * d + col] = p[0][tid];
        __syncthreads();
    }
}

// a wave per packed pair of the call
__global__ __launch_bounds__(BLK) void k_fcov_cross(const CSeg *__restrict__ segs, const int32_t *__restrict__ ent_seg, int64_t P, int64_t d,
                                                    int64_t ntiles, const double *__restrict__ w, const double *__restrict__ f,
                                                    double *__restrict__ cross)
{
    const int lane = threadIdx.x & 63;
    const int64_t e = (int64_t)blockIdx.x * (BLK / WAVE) + (threadIdx.x >> 6);
    if (e >= P) return;                                                // whole waves leave
    const CSeg s = segs[ent_seg[e]];
    const int L = s.L, pr = (int)(e - s.pair0);
    int lo, hi;
    pair_of(pr, L, lo, hi);
    const double *fa = f + (s.col0 + lo) * d, *fb = f + (s.col0 + hi) * d;
    double acc = 0.0;
    for (int64_t t = lane; t < ntiles; t += WAVE) {
        const int64_t c0 = t * TILE;
        const int tw = (int)min((int64_t)TILE, d - c0);
        double x = 0.0;
        for (int c = 0; c < tw; c++) x = fma(w[c0 + c] * fa[c0 + c], fb[c0 + c], x);
        acc += x;
    }
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) acc += __shfl_down(acc, off, WAVE);
    if (lane == 0) cross[s.pair0 + lo * L - lo * (lo - 1) / 2 + (hi - lo)] = acc;
}

}  // namespace

extern "C" int bluest_field_group_moments(int64_t S, int64_t d, const int64_t *counts, const int32_t *sizes, const double *const *values,
                                          const double *w, double *second, double *cross, double *first, void *stream)
{
    if (S < 1) return fail(BLUEST_ERR_ARG, "S=%lld: at least one segment is needed", (long long)S);
    if (d < 1) return fail(BLUEST_ERR_ARG, "d=%lld: at least one component is needed", (long long)d);
    if (!counts || !sizes || !values || !w || !second || !cross) return fail(BLUEST_ERR_ARG, "null pointer");
    const int64_t ntiles = (d - 1) / TILE + 1;
    int64_t T = 0, P = 0, nchunks = 0;
    double npartp = 0.0, npartf = 0.0, nwg = 0.0;
    int Lmax = 1;
    for (int64_t s = 0; s < S; s++) {
        int rc = check_segment(s, counts, sizes, values); if (rc) return rc;
        const int L = sizes[s];
        const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
        const int tb = field_cov_tiles(L, ntiles);
        T += L;
        P += L * (L + 1) / 2;
        nchunks += nc;
        Lmax = std::max(Lmax, L);
        npartp += (double)nc * (double)ntiles * (L * (L + 1) / 2);
        npartf += (double)nc * (double)d * L * CLASSES;
        nwg += (double)nc * (double)((ntiles - 1) / tb + 1);
    }
    if (T > 0x7fffffffLL || nchunks > 0x7fffffffLL || (double)T * (double)d > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 columns, column-components (T d) or chunks of %d samples in one call", GCHUNK);
    if (P > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 packed pairs in one call");
    if (npartp > 2147483647.0 || npartf > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 partial sums ((pair, chunk, tile) or (chunk, column, component)) in one call");
    if (nwg > 2147483647.0) return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 (chunk, block of tiles) workgroups in one call");
    for (int64_t c = 0; c < d; c++)
        if (!(w[c] >= 0.0) || std::isinf(w[c])) return fail(BLUEST_ERR_ARG, "w[%lld]=%g: the weights must be finite and >= 0", (long long)c, w[c]);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;

    // ---- the tables: segments, the segment of every packed pair ----
    std::vector<CSeg> segs((size_t)S);
    std::vector<int32_t> ent_seg((size_t)P);
    std::vector<int64_t> shift_at((size_t)S, -1);      // host segments: where the first-sample row [L d] lies in the shift buffer
    std::vector<char> device((size_t)S), staged((size_t)S);
    std::vector<size_t> row_bytes((size_t)S);
    std::vector<int> key_of((size_t)S), sb_of((size_t)S);
    size_t lds_of[TB_KEYS] = {0, 0, 0, 0, 0};
    int64_t nshift = 0, n_partp = 0, n_partf = 0;
    {
        int64_t col = 0, pair = 0;
        for (int64_t s = 0; s < S; s++) {
            const int L = sizes[s], tri = L * (L + 1) / 2;
            const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
            const int tb = field_cov_tiles(L, ntiles), sb = field_cov_rows(L, tb);
            int key = 0;
            while ((1 << key) < tb) key++;
            key_of[s] = key;
            sb_of[s] = sb;
            lds_of[key] = std::max(lds_of[key], ((size_t)sb * tb * L * STR + (size_t)L * tb * TILE) * 8);
            segs[s] = CSeg{n_partp, n_partf, nc, pair, col, L, 0};
            std::fill(ent_seg.begin() + pair, ent_seg.begin() + pair + tri, (int32_t)s);
            col += L;
            pair += tri;
            n_partp += nc * ntiles * tri;
            n_partf += nc * L * d * CLASSES;
            device[s] = counts[s] > 0 && on_device(values[s]);
            staged[s] = counts[s] > 0 && !device[s];
            row_bytes[s] = (size_t)L * d * 8;
            if (staged[s]) {
                shift_at[s] = nshift;
                nshift += L * d;
            }
        }
    }
    std::vector<double> shifts((size_t)nshift);
    for (int64_t s = 0; s < S; s++)
        if (shift_at[s] >= 0) std::memcpy(shifts.data() + shift_at[s], values[s], (size_t)sizes[s] * d * 8);

    const SlabPlan plan = plan_slabs(S, counts, row_bytes.data(), staged.data(), GCHUNK, (size_t)slab_budget());

    DeviceArena arena;
    const size_t b_pairs = (size_t)P * 8, b_first = (size_t)T * d * 8;
    const size_t o_stage = arena.take(plan.stage_bytes + 256), o_shift = arena.take((size_t)nshift * 8), o_partp = arena.take((size_t)n_partp * 8),
                 o_partf = arena.take((size_t)n_partf * 8), o_chunks = arena.take((size_t)nchunks * sizeof(CChunk)),
                 o_segs = arena.take((size_t)S * sizeof(CSeg)), o_ents = arena.take((size_t)P * 4), o_w = arena.take((size_t)d * 8),
                 o_f = arena.take(b_first), o_second = arena.take(b_pairs), o_cross = arena.take(b_pairs);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_stage = (const double *)(dv + o_stage), *d_shift = (const double *)(dv + o_shift), *d_w = (const double *)(dv + o_w);
    double *d_partp = (double *)(dv + o_partp), *d_partf = (double *)(dv + o_partf), *d_f = (double *)(dv + o_f);
    double *d_second = (double *)(dv + o_second), *d_cross = (double *)(dv + o_cross);
    const CChunk *d_chunks = (const CChunk *)(dv + o_chunks);
    const CSeg *d_segs = (const CSeg *)(dv + o_segs);
    const int32_t *d_ents = (const int32_t *)(dv + o_ents);

    // ---- the chunks: launch group 0 reads the device segments where they lie, group 1 + k the pieces of slab k; a list per TB ----
    ChunkLists<CChunk> chunks(1 + plan.slab_used.size(), TB_KEYS, nchunks);
    auto add_chunks = [&](size_t g, int64_t s, const double *base, int64_t first_row, int64_t rows, const double *shift) {
        const int L = sizes[s];
        const int64_t W = (int64_t)L * d;
        for (int64_t a = 0; a < rows; a += GCHUNK) {
            const int64_t c = (first_row + a) / GCHUNK;
            chunks.add(g, (size_t)key_of[s], CChunk{base + a * W, shift, segs[s].partp + c * ntiles, segs[s].nchunks * ntiles, segs[s].partf + c * CLASSES * W,
                                                    (int32_t)std::min<int64_t>(GCHUNK, rows - a), L, sb_of[s], 0});
        }
    };
    for (int64_t s = 0; s < S; s++)
        if (device[s]) add_chunks(0, s, values[s], 0, counts[s], values[s]);
    for (const Piece &pc : plan.pieces) add_chunks(1 + (size_t)pc.slab, pc.seg, d_stage + pc.at / 8, pc.first, pc.rows, d_shift + shift_at[pc.seg]);
    rc = chunks.flatten(); if (rc) return rc;
    // the tables lie side by side on the device: one image of them on the host, one copy
    std::vector<char> tables(o_f - o_chunks);
    if (nchunks > 0) std::memcpy(tables.data(), chunks.table.data(), (size_t)nchunks * sizeof(CChunk));
    std::memcpy(tables.data() + (o_segs - o_chunks), segs.data(), (size_t)S * sizeof(CSeg));
    std::memcpy(tables.data() + (o_ents - o_chunks), ent_seg.data(), (size_t)P * 4);
    std::memcpy(tables.data() + (o_w - o_chunks), w, (size_t)d * 8);
    HIP_TRY(hipMemcpyAsync(dv + o_chunks, tables.data(), tables.size(), hipMemcpyHostToDevice, st));
    if (nshift > 0) HIP_TRY(hipMemcpyAsync(dv + o_shift, shifts.data(), (size_t)nshift * 8, hipMemcpyHostToDevice, st));

    auto launch_group = [&](size_t g) -> hipError_t {
        for (int key = 0; key < TB_KEYS; key++) {
            const size_t c0 = chunks.begin(g, (size_t)key), c1 = chunks.end(g, (size_t)key);
            if (c1 <= c0) continue;
            const int64_t nblocks = (ntiles - 1) / (1 << key) + 1;
            hipLaunchKernelGGL(k_fcov_partial, dim3((unsigned)((int64_t)(c1 - c0) * nblocks)), dim3(BLK), lds_of[key], st, d_chunks + c0, d,
                               ntiles, nblocks, key, d_w, d_partp, d_partf);
            const hipError_t e = hipGetLastError();
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    rc = run_slabs(plan, dv + o_stage, values, counts, row_bytes.data(), 1, launch_group, st); if (rc) return rc;

    const dim3 gp((unsigned)((P + BLK / WAVE - 1) / (BLK / WAVE)));
    hipLaunchKernelGGL(k_fcov_fold_second, gp, dim3(BLK), 0, st, d_segs, d_ents, P, ntiles, (const double *)d_partp, d_second);
    HIP_TRY(hipGetLastError());
    const dim3 gf((unsigned)S, (unsigned)std::min<int64_t>(((int64_t)Lmax * d + FOLD_COLS - 1) / FOLD_COLS, 65535));
    hipLaunchKernelGGL(k_fcov_fold_first, gf, dim3(BLK), 0, st, d_segs, d, (const double *)d_partf, d_f);
    HIP_TRY(hipGetLastError());
    hipLaunchKernelGGL(k_fcov_cross, gp, dim3(BLK), 0, st, d_segs, d_ents, P, d, ntiles, d_w, (const double *)d_f, d_cross);
    HIP_TRY(hipGetLastError());
    std::vector<char> results(o_cross - o_second + b_pairs);              // `second` and `cross` lie side by side: one copy back
    std::vector<double> f_host(first ? (size_t)T * d : 0);
    HIP_TRY(hipMemcpyAsync(results.data(), d_second, results.size(), hipMemcpyDeviceToHost, st));
    if (first) HIP_TRY(hipMemcpyAsync(f_host.data(), d_f, b_first, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(second, results.data(), b_pairs);
    std::memcpy(cross, results.data() + (o_cross - o_second), b_pairs);
    if (first) std::memcpy(first, f_host.data(), b_first);
    return BLUEST_OK;
}

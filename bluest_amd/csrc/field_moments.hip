// field_moments.hip -- Part 15 of include/bluest_hip.h: per (segment, component) the sum and the sum of squares over the samples of
// z_i[c] = sum_j coef_j (y_ij[c] - y_0j[c]), the BLUE-weighted combination of a group's models: what the sampled variance of every
// component of a field estimate is made of.
//
// The segments, the chunk table and the slabs of staged host data are those of staging.hpp, the fold over the chunks is that of
// fields.hip; the first-sample rows of the host segments travel in a buffer of their own, as in moments.hip, so a chunk in a later
// slab still finds its segment's shift.  What is its own is the work of a chunk.  A row of a segment is W = L d contiguous doubles,
// [model j][component c], and the chain of z over j walks it with stride d.  Per call one k_fmom_* launch per slab (device
// segments: one launch for all of them; two where only some segments take the split form of k_fmom_wide) and one k_fmom_fold,
// no atomics, nothing sized by the device.  The shape follows d and W (field_moments_rows and field_moments_split, decided on
// the host; the chunk table carries sb, the segment table the split):
//   d >= 64     k_fmom_wide    1-D grid over (chunk, block of 64 components), 512 threads = 8 classes x 64 components.  The block's
//                              part of the shift row, [L][64], is staged in LDS (at most 32 KB); a thread then reads its class's
//                              sixteen rows straight from memory, 512-byte runs along c per wave and model, forms z of four rows
//                              side by side in registers (the fma chains over j) and takes q += z, qq = fma(z, z, qq) row by row.
//                              The class sums meet in LDS and join in the fixed tree.
//               <SPLIT>        64 <= d < 1024 and L >= 16 (field_moments_split): a chunk has fewer than 16 blocks of components and
//                              a workgroup would read 1 MB and more alone, so every class gets a workgroup of 256 threads: wave w
//                              forms z of the class's rows 4 w .. 4 w + 3 into LDS, wave 0 adds the class in ascending order, the
//                              eight class sums of a chunk go to memory and k_fmom_fold joins them in the tree.
//   d <  64     k_fmom_staged  one workgroup of 256 threads per chunk walks it in SUB-BLOCKS of sb consecutive rows, sb the largest
//                              power of two <= 128 with sb (W' + d) + 16 d <= 4096 doubles of LDS (32 KB: five workgroups per
//                              compute unit), at least 1 (W = 4032, d = 63: 40 KB).  A sub-block is staged as stage_shifted of
//                              moments.hip stages a chunk: 16-byte loads from the first 16-byte boundary on, the shift subtracted
//                              on the way (one rounding per value); a row takes W' = W | 1 doubles, so that the rows, which
//                              consecutive lanes read at d = 1, lie on different banks.  Then a thread per (row, component) runs
//                              the fma chain over j from LDS and leaves z in LDS, and a thread per (class, component) adds the
//                              class's rows of the sub-block in ascending order.  With sb >= 16 a sub-block holds whole classes
//                              (small W: sb = 128 up to W' + d + d / 8 <= 32, the whole chunk at once); with sb < 16 it lies inside
//                              one class, and the thread of a component carries q and qq in registers from one sub-block to the next.
//                              sb halves wherever (4096 - 16 d) / (W' + d) falls below it: at d = 1 from 128 to 64 between
//                              L = 29 and 30, at d = 63 from 16 (L <= 2) down to 1 (L >= 24).
//   k_fmom_fold                grid (segment, block of 64 of the 2 d sums), as k_fsum_fold of fields.hip: wave g = 0..3 computes the
//                              lane sums l = g, g + 4, ... of Part 11 step 3 for its 64 sums into LDS, coalesced along c, then the
//                              tree runs over LDS.
// The shape never enters the order of the additions: z of a (row, component) is one chain whoever runs it, and every class is added
// row by row from +0.0 by one thread.  Every value is read once; a chunk writes 2 d doubles.
#include "staging.hpp"
#include "field_partials.hpp"

namespace {

using bluest_partials::ZChunk;
using bluest_partials::field_moments_rows;
using bluest_partials::field_moments_split;

constexpr int BLK = 256;                            // k_fmom_staged, k_fmom_fold
constexpr int WIDE_COLS = WAVE;                     // components per workgroup of k_fmom_wide, and the least d it takes
constexpr int WIDE_BLK = CLASSES * WIDE_COLS;
constexpr int STAGE_DOUBLES = 4096;                 // LDS of a k_fmom_staged workgroup where one row fits it
constexpr int FOLD_COLS = 64;
constexpr int SPLIT_FROM_L = 16, SPLIT_BELOW_D = 16 * WIDE_COLS;
constexpr int LOADS = 4;                            // 16-byte loads a thread keeps in flight while it stages
static_assert((size_t)BLUEST_MAX_MODELS * WIDE_COLS * 8 + 2 * WIDE_BLK * 8 <= 64 * 1024, "shift and class sums of k_fmom_wide fit the default LDS");
static_assert(CLASSES * (WIDE_COLS - 1) <= 2 * BLK, "two passes of k_fmom_staged cover every (class, component)");

__host__ __device__ constexpr int padded_row(int W) { return W | 1; }
__host__ __device__ constexpr int staged_doubles(int W, int d, int sb) { return sb * (padded_row(W) + d) + 2 * CLASSES * d; }
static_assert((size_t)staged_doubles(BLUEST_MAX_MODELS * (WIDE_COLS - 1), WIDE_COLS - 1, 1) * 8 <= 64 * 1024, "one row of the widest staged segment fits the default LDS");

struct ZSeg {
    int64_t part;           // first chunk's partial sums
    int64_t nchunks;
    int64_t split;          // 1: a chunk's partial sums are its eight class sums [class][2 d], still to be joined
};

// z of the rows r, r + 1, r + 2, r + 3 of one component, their chains side by side: the loads of four rows are in flight together
__device__ __forceinline__ void chains4(const double *p, int64_t W, int64_t d, int L, const double *sh, const double *__restrict__ cf,
                                        double (&z)[4])
{
    z[0] = z[1] = z[2] = z[3] = 0.0;
#pragma unroll 8
    for (int j = 0; j < L; j++) {                                       // (32 loads in flight per thread: a wave per SIMD keeps the memory busy)
        const double a = sh[j * WIDE_COLS], cj = cf[j];
        const double *pj = p + (int64_t)j * d;
        z[0] = fma(cj, pj[0] - a, z[0]);
        z[1] = fma(cj, pj[W] - a, z[1]);
        z[2] = fma(cj, pj[2 * W] - a, z[2]);
        z[3] = fma(cj, pj[3 * W] - a, z[3]);
    }
}

__device__ __forceinline__ double chain1(const double *p, int64_t d, int L, const double *sh, const double *__restrict__ cf)
{
    double z = 0.0;
#pragma unroll 4
    for (int j = 0; j < L; j++) z = fma(cf[j], p[(int64_t)j * d] - sh[j * WIDE_COLS], z);
    return z;
}

// SPLIT false: grid (chunks of the launch) * ncb, ncb = ceil(d / 64); 512 threads, wave k takes class k.
// SPLIT true:  grid (chunks of the launch) * ncb * 8, one workgroup of 256 threads per class: wave w forms z of the class's rows
//              4 w .. 4 w + 3 and leaves it in LDS, then wave 0 adds the class's rows in ascending order; the chunk's eight class
//              sums go to memory as they are, and k_fmom_fold joins them in the tree.
template <bool SPLIT>
__global__ __launch_bounds__(SPLIT ? BLK : WIDE_BLK) void k_fmom_wide(const ZChunk *__restrict__ table, const double *__restrict__ coef,
                                                                      int64_t d, int64_t ncb, double *__restrict__ part)
{
    constexpr int B = SPLIT ? BLK : WIDE_BLK;
    extern __shared__ double lds[];
    const int64_t b = SPLIT ? blockIdx.x / CLASSES : blockIdx.x, local = b / ncb, cb = b - local * ncb;
    const ZChunk ch = table[local];
    const int tid = threadIdx.x, wave = tid >> 6, lane = tid & 63, L = ch.L;
    const int k = SPLIT ? (int)(blockIdx.x % CLASSES) : wave;           // the class of this thread
    const int64_t c0 = cb * WIDE_COLS, W = (int64_t)L * d;
    const int bw = (int)min((int64_t)WIDE_COLS, d - c0);
    double *sh = lds, *buf = lds + L * WIDE_COLS;                       // [L][64]; [class][sum, square][64] or, SPLIT, z [16][64]
    const int r0 = k * CLASS_ROWS, r1 = min(r0 + CLASS_ROWS, ch.rows);
    if (!SPLIT || r0 < r1)
        for (int t = tid; t < L * WIDE_COLS; t += B) {
            const int j = t >> 6, c = t & 63;
            if (c < bw) sh[t] = ch.shift[(int64_t)j * d + c0 + c];
        }
    __syncthreads();
    const double *cf = coef + ch.col0, *src = ch.src + c0 + lane;
    double q = 0.0, qq = 0.0, z[4];
    if (SPLIT) {
        const int a = r0 + 4 * wave;
        if (lane < bw && a < r1) {
            if (a + 4 <= r1) chains4(src + (int64_t)a * W, W, d, L, sh + lane, cf, z);
            else {
#pragma unroll
                for (int i = 0; i < 3; i++)
                    if (a + i < r1) z[i] = chain1(src + (int64_t)(a + i) * W, d, L, sh + lane, cf);
            }
#pragma unroll
            for (int i = 0; i < 4; i++)
                if (a + i < r1) buf[(4 * wave + i) * WIDE_COLS + lane] = z[i];
        }
        __syncthreads();
        if (wave == 0 && lane < bw) {
            for (int r = 0; r < r1 - r0; r++) {
                const double zr = buf[r * WIDE_COLS + lane];
                q += zr;
                qq = fma(zr, zr, qq);
            }
            double *dst = part + ch.part + (int64_t)k * 2 * d + c0 + lane;      // [class][sum, square][d]
            dst[0] = q;
            dst[d] = qq;
        }
    } else {
        if (lane < bw) {
            int r = r0;
            for (; r + 4 <= r1; r += 4) {
                chains4(src + (int64_t)r * W, W, d, L, sh + lane, cf, z);
#pragma unroll
                for (int i = 0; i < 4; i++) {
                    q += z[i];
                    qq = fma(z[i], z[i], qq);
                }
            }
            for (; r < r1; r++) {
                const double zr = chain1(src + (int64_t)r * W, d, L, sh + lane, cf);
                q += zr;
                qq = fma(zr, zr, qq);
            }
        }
        buf[(2 * k) * WIDE_COLS + lane] = q;
        buf[(2 * k + 1) * WIDE_COLS + lane] = qq;
        __syncthreads();
        if (tid < 2 * WIDE_COLS) {
            const int which = tid >> 6;                                 // 0: the sums, 1: the squares
            if (lane < bw) part[ch.part + which * d + c0 + lane] = class_tree(buf + which * WIDE_COLS + lane, 2 * WIDE_COLS);
        }
    }
}

// rows [0, nsb) of `src` as d = value - shift, row r at tile + r * WP
__device__ __forceinline__ void stage_rows(double *tile, const double *__restrict__ src, const double *__restrict__ sh, int nsb, int W,
                                           int WP, int tid)
{
    const int cnt = nsb * W;
    // src is 8-byte aligned: one value in front when it is not 16-byte aligned, pairs from there, one value behind when one is left
    const int head = (int)(((uintptr_t)src >> 3) & 1);
    const int npair = (cnt - head) >> 1;
    const double2 *pairs = (const double2 *)(src + head);
    const int step = (2 * BLK) % W, rstep = (2 * BLK) / W;
    int row = (head + 2 * tid) / W, j = (head + 2 * tid) - row * W;    // where element head + 2 i lies
    for (int i0 = tid; i0 < npair; i0 += LOADS * BLK) {
        double2 v[LOADS];
#pragma unroll
        for (int u = 0; u < LOADS; u++)
            if (i0 + u * BLK < npair) v[u] = pairs[i0 + u * BLK];
#pragma unroll
        for (int u = 0; u < LOADS; u++) {
            if (i0 + u * BLK < npair) {
                const bool wrap = j + 1 == W;
                const int j1 = wrap ? 0 : j + 1, row1 = wrap ? row + 1 : row;
                tile[row * WP + j] = v[u].x - sh[j];
                tile[row1 * WP + j1] = v[u].y - sh[j1];
                j += step;
                row += rstep;
                if (j >= W) { j -= W; row++; }
            }
        }
    }
    if (tid == 0) {
        if (head) tile[0] = src[0] - sh[0];
        if ((cnt - head) & 1) tile[(nsb - 1) * WP + W - 1] = src[cnt - 1] - sh[W - 1];
    }
}

// grid: the chunks of the launch
__global__ __launch_bounds__(BLK) void k_fmom_staged(const ZChunk *__restrict__ table, const double *__restrict__ coef, int d,
                                                     double *__restrict__ part)
{
    extern __shared__ double lds[];
    const ZChunk ch = table[blockIdx.x];
    const int tid = threadIdx.x, L = ch.L, W = L * d, WP = padded_row(W), sb = ch.sb;
    double *cls = lds, *zt = cls + 2 * CLASSES * d, *tile = zt + sb * d;    // [class][sum, square][d], [sb][d], [sb][WP]
    const double *cf = coef + ch.col0;
    for (int t = tid; t < 2 * CLASSES * d; t += BLK) cls[t] = 0.0;         // (a class without rows stays +0.0)
    double q = 0.0, qq = 0.0;                                               // sb < 16: the running class of component tid
    for (int sub = 0; sub < ch.rows; sub += sb) {
        const int nsb = min(sb, ch.rows - sub);
        __syncthreads();                                                    // every read of the last sub-block is done
        stage_rows(tile, ch.src + (int64_t)sub * W, ch.shift, nsb, W, WP, tid);
        __syncthreads();
        for (int p = tid; p < nsb * d; p += BLK) {                          // z of (row, component), component fastest
            const int r = p / d, c = p - r * d;
            const double *v = tile + r * WP + c;
            double z = 0.0;
#pragma unroll 4
            for (int j = 0; j < L; j++) z = fma(cf[j], v[j * d], z);
            zt[p] = z;
        }
        __syncthreads();
        if (sb >= CLASS_ROWS) {                                             // whole classes: a thread per (class of the sub-block, component)
            const int kc = (nsb + CLASS_ROWS - 1) / CLASS_ROWS;
            for (int p = tid; p < kc * d; p += BLK) {
                const int kk = p / d, c = p - kk * d;
                const int r1 = min((kk + 1) * CLASS_ROWS, nsb);
                double a = 0.0, aa = 0.0;
                for (int r = kk * CLASS_ROWS; r < r1; r++) {
                    const double z = zt[r * d + c];
                    a += z;
                    aa = fma(z, z, aa);
                }
                const int k = sub / CLASS_ROWS + kk;
                cls[(2 * k) * d + c] = a;
                cls[(2 * k + 1) * d + c] = aa;
            }
        } else if (tid < d) {                                               // inside one class: the sums wait in registers
            if ((sub & (CLASS_ROWS - 1)) == 0) q = qq = 0.0;
            for (int r = 0; r < nsb; r++) {
                const double z = zt[r * d + tid];
                q += z;
                qq = fma(z, z, qq);
            }
            const int k = sub / CLASS_ROWS;
            cls[(2 * k) * d + tid] = q;                                     // (the class's last sub-block writes last)
            cls[(2 * k + 1) * d + tid] = qq;
        }
    }
    __syncthreads();
    for (int x = tid; x < 2 * d; x += BLK) part[ch.part + x] = class_tree(cls + x, 2 * d);     // x < d: the sums, then the squares
}

// grid (segment, block of 64 of the 2 d sums of a chunk)
__global__ __launch_bounds__(BLK) void k_fmom_fold(const ZSeg *__restrict__ segs, const double *__restrict__ part, int64_t d,
                                                   double *__restrict__ zsum, double *__restrict__ zsq)
{
    __shared__ double p[WAVE][FOLD_COLS];
    const ZSeg sg = segs[blockIdx.x];
    const int tid = threadIdx.x, g = tid >> 6, j = tid & 63;
    const int64_t W2 = 2 * d, step = sg.split ? CLASSES * W2 : W2;
    for (int64_t col0 = (int64_t)blockIdx.y * FOLD_COLS; col0 < W2; col0 += (int64_t)gridDim.y * FOLD_COLS) {
        const int64_t col = col0 + j;
        for (int l = g; l < WAVE; l += BLK / WAVE) {
            double acc = 0.0;
            if (col < W2)
                for (int64_t c = l; c < sg.nchunks; c += WAVE) {
                    const double *pc = part + sg.part + c * step + col;
                    acc += sg.split ? class_tree(pc, (int)W2) : pc[0];
                }
            p[l][j] = acc;
        }
        __syncthreads();
        for (int off = 32; off > 0; off >>= 1) {                       // lane l < off takes p_l + p_(l + off)
            for (int v = tid; v < off * FOLD_COLS; v += BLK) p[v >> 6][v & 63] += p[(v >> 6) + off][v & 63];
            __syncthreads();
        }
        if (tid < FOLD_COLS && col < W2) {
            if (col < d) zsum[(int64_t)blockIdx.x * d + col] = p[0][tid];
            else zsq[(int64_t)blockIdx.x * d + col - d] = p[0][tid];
        }
        __syncthreads();
    }
}

}  // namespace

// k_fmom_wide with a workgroup per class: where a chunk has fewer than 16 blocks of components and a workgroup would otherwise
// read 1 MB and more on its own (the eight class sums that then go through memory are 1 / (8 L) of what the chunk reads)
bool bluest_partials::field_moments_split(int L, int64_t d) { return d >= WIDE_COLS && d < SPLIT_BELOW_D && L >= SPLIT_FROM_L; }

// rows per sub-block of k_fmom_staged; 0: k_fmom_wide
int bluest_partials::field_moments_rows(int L, int64_t d)
{
    if (d >= WIDE_COLS) return 0;
    int sb = GCHUNK;
    while (sb > 1 && staged_doubles(L * (int)d, (int)d, sb) > STAGE_DOUBLES) sb >>= 1;
    return sb;
}

int bluest_partials::field_moments_lds(int L, int64_t d)
{
    return d >= WIDE_COLS ? L * WIDE_COLS + 2 * WIDE_BLK : staged_doubles(L * (int)d, (int)d, field_moments_rows(L, d));
}

hipError_t bluest_partials::launch_fmom_partial(const ZChunk *table, size_t n, bool split, int lds_doubles, int64_t d, const double *coef,
                                                double *part, hipStream_t st)
{
    if (n == 0) return hipSuccess;
    const size_t lds = (size_t)lds_doubles * 8;
    const int64_t ncb = (d + WIDE_COLS - 1) / WIDE_COLS, nblk = (int64_t)n * ncb;
    if (split) hipLaunchKernelGGL(k_fmom_wide<true>, dim3((unsigned)(nblk * CLASSES)), dim3(BLK), lds, st, table, coef, d, ncb, part);
    else if (d >= WIDE_COLS) hipLaunchKernelGGL(k_fmom_wide<false>, dim3((unsigned)nblk), dim3(WIDE_BLK), lds, st, table, coef, d, ncb, part);
    else hipLaunchKernelGGL(k_fmom_staged, dim3((unsigned)n), dim3(BLK), lds, st, table, coef, (int)d, part);
    return hipGetLastError();
}

extern "C" int bluest_field_weighted_moments(int64_t S, int64_t d, const int64_t *counts, const int32_t *sizes,
                                             const double *const *values, const double *coef, double *zsum, double *zsq, void *stream)
{
    if (S < 1) return fail(BLUEST_ERR_ARG, "S=%lld: at least one segment is needed", (long long)S);
    if (d < 1) return fail(BLUEST_ERR_ARG, "d=%lld: at least one component is needed", (long long)d);
    if (!counts || !sizes || !values || !coef || !zsum || !zsq) return fail(BLUEST_ERR_ARG, "null pointer");
    int64_t T = 0, nchunks = 0;
    for (int64_t s = 0; s < S; s++) {
        int rc = check_segment(s, counts, sizes, values); if (rc) return rc;
        T += sizes[s];
        nchunks += (counts[s] + GCHUNK - 1) / GCHUNK;
    }
    const int64_t ncb = (d + WIDE_COLS - 1) / WIDE_COLS;
    if (T > 0x7fffffffLL || nchunks > 0x7fffffffLL || (double)T * (double)d > 2147483647.0 || (double)S * (double)d > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 columns, column-components (T d), values (S d) or chunks of %d samples in one call", GCHUNK);
    if ((double)nchunks * (double)ncb * CLASSES > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 (chunk, block of %d components, class) workgroups in one call", WIDE_COLS);
    for (int64_t t = 0; t < T; t++)
        if (!std::isfinite(coef[t])) return fail(BLUEST_ERR_ARG, "coef[%lld]=%g is not finite", (long long)t, coef[t]);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    // ---- the tables: segments ----
    std::vector<ZSeg> segs((size_t)S);
    std::vector<int64_t> col0((size_t)S), shift_at((size_t)S, -1);    // host segments: where the first-sample row [L d] lies in the shift buffer
    std::vector<char> device((size_t)S), staged((size_t)S);
    std::vector<size_t> row_bytes((size_t)S);
    int64_t nshift = 0, npart = 0;
    {
        int64_t col = 0;
        for (int64_t s = 0; s < S; s++) {
            const int64_t nc = (counts[s] + GCHUNK - 1) / GCHUNK;
            const int64_t per_chunk = 2 * d * (field_moments_split(sizes[s], d) ? CLASSES : 1);
            segs[s] = ZSeg{npart, nc, per_chunk != 2 * d};
            col0[s] = col;
            col += sizes[s];
            npart += nc * per_chunk;
            device[s] = counts[s] > 0 && on_device(values[s]);
            staged[s] = counts[s] > 0 && !device[s];
            row_bytes[s] = (size_t)sizes[s] * d * 8;
            if (staged[s]) {
                shift_at[s] = nshift;
                nshift += sizes[s] * d;
            }
        }
    }
    std::vector<double> shifts((size_t)nshift);
    for (int64_t s = 0; s < S; s++)
        if (shift_at[s] >= 0) std::memcpy(shifts.data() + shift_at[s], values[s], (size_t)sizes[s] * d * 8);

    const SlabPlan plan = plan_slabs(S, counts, row_bytes.data(), staged.data(), GCHUNK, (size_t)slab_budget());
    const size_t n_groups = 1 + plan.slab_used.size();

    DeviceArena arena;
    const size_t b_out = (size_t)S * d * 8;
    const size_t o_stage = arena.take(plan.stage_bytes + 256), o_shift = arena.take((size_t)nshift * 8), o_part = arena.take((size_t)npart * 8),
                 o_chunks = arena.take((size_t)nchunks * sizeof(ZChunk)), o_segs = arena.take((size_t)S * sizeof(ZSeg)),
                 o_coef = arena.take((size_t)T * 8), o_zsum = arena.take(b_out), o_zsq = arena.take(b_out);
    HIP_TRY(arena.alloc());
    char *dv = arena.base;
    const double *d_stage = (const double *)(dv + o_stage), *d_shift = (const double *)(dv + o_shift), *d_coef = (const double *)(dv + o_coef);
    double *d_part = (double *)(dv + o_part), *d_zsum = (double *)(dv + o_zsum), *d_zsq = (double *)(dv + o_zsq);
    ZChunk *d_chunks = (ZChunk *)(dv + o_chunks);

    // ---- the chunks: launch group 0 reads the device segments where they lie, group 1 + k the pieces of slab k; the split
    // segments of a group have a list of their own ----
    ChunkLists<ZChunk> chunks(n_groups, 2, nchunks);
    std::vector<int> lds_doubles(2 * n_groups, 0);
    auto add_chunks = [&](size_t g, int64_t s, const double *base, int64_t first_row, int64_t rows, const double *shift) {
        const int L = sizes[s], sb = field_moments_rows(L, d);
        const int64_t W = (int64_t)L * d, per_chunk = segs[s].split ? 2 * d * CLASSES : 2 * d;
        int &lds = lds_doubles[2 * g + (size_t)segs[s].split];
        lds = std::max(lds, bluest_partials::field_moments_lds(L, d));
        for (int64_t a = 0; a < rows; a += GCHUNK)
            chunks.add(g, (size_t)segs[s].split, ZChunk{base + a * W, shift, segs[s].part + ((first_row + a) / GCHUNK) * per_chunk,
                                                        (int32_t)std::min<int64_t>(GCHUNK, rows - a), L, (int32_t)col0[s], sb});
    };
    for (int64_t s = 0; s < S; s++)
        if (device[s]) add_chunks(0, s, values[s], 0, counts[s], values[s]);
    for (const Piece &pc : plan.pieces) add_chunks(1 + (size_t)pc.slab, pc.seg, d_stage + pc.at / 8, pc.first, pc.rows, d_shift + shift_at[pc.seg]);
    rc = chunks.flatten(); if (rc) return rc;
    // the tables lie side by side on the device: one image of them on the host, one copy
    std::vector<char> tables(o_zsum - o_chunks);
    if (nchunks > 0) std::memcpy(tables.data(), chunks.table.data(), (size_t)nchunks * sizeof(ZChunk));
    std::memcpy(tables.data() + (o_segs - o_chunks), segs.data(), (size_t)S * sizeof(ZSeg));
    std::memcpy(tables.data() + (o_coef - o_chunks), coef, (size_t)T * 8);
    HIP_TRY(hipMemcpyAsync(dv + o_chunks, tables.data(), tables.size(), hipMemcpyHostToDevice, st));
    if (nshift > 0) HIP_TRY(hipMemcpyAsync(dv + o_shift, shifts.data(), (size_t)nshift * 8, hipMemcpyHostToDevice, st));

    auto launch_group = [&](size_t g) -> hipError_t {
        for (size_t split = 0; split < 2; split++) {
            const size_t c0 = chunks.begin(g, split), c1 = chunks.end(g, split);
            const hipError_t e = bluest_partials::launch_fmom_partial(d_chunks + c0, c1 - c0, split != 0, lds_doubles[2 * g + split], d, d_coef,
                                                                      d_part, st);
            if (e != hipSuccess) return e;
        }
        return hipSuccess;
    };
    rc = run_slabs(plan, dv + o_stage, values, counts, row_bytes.data(), 1, launch_group, st); if (rc) return rc;
    const dim3 gf((unsigned)S, (unsigned)std::min<int64_t>((2 * d + FOLD_COLS - 1) / FOLD_COLS, 65535));
    hipLaunchKernelGGL(k_fmom_fold, gf, dim3(BLK), 0, st, (const ZSeg *)(dv + o_segs), (const double *)d_part, d, d_zsum, d_zsq);
    HIP_TRY(hipGetLastError());
    std::vector<char> results(o_zsq - o_zsum + b_out);                    // zsum and zsq lie side by side too: one copy back
    HIP_TRY(hipMemcpyAsync(results.data(), d_zsum, results.size(), hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    std::memcpy(zsum, results.data(), b_out);
    std::memcpy(zsq, results.data() + (o_zsq - o_zsum), b_out);
    return BLUEST_OK;
}

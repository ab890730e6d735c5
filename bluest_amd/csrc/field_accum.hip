// field_accum.hip -- Part 19 of include/bluest_hip.h: ONE segment of one field output, delivered in pieces over many calls, to the
// bits of bluest_field_sums and bluest_field_weighted_moments on the whole segment.
//
// The order contract of Parts 11, 12 and 15 makes the running state small.  A chunk's value depends on its own rows (and, for the
// moments, on the segment's first row); chunk c belongs to lane c mod 64, which adds its chunks in ascending order from +0.0; a
// tree joins the lanes.  So the handle keeps, on the device,
//   lanes_s [64][W]      the lane partials of the sums, W = L d           lanes_m [64][2 d]   those of zsum | zsq
//   first   [W]          the segment's first row, the shift of Part 15    tail    [128][W]    the rows of the unfinished chunk
// and a grow-only scratch for one update: the per-chunk partials, the two chunk tables and the staging buffer of a host batch.
// An update completes the tail's chunk inside the tail buffer, reads the whole chunks of a device batch where they lie (those of a
// host batch slab by slab from the staging buffer, under the budget of bluest_group_sums_slab), runs the partial kernels of
// fields.hip and field_moments.hip over them (field_partials.hpp), and then
//   k_faccum_carry   grid (block of columns, touched lane i = 0 .. min(nc, 64) - 1): the update's chunks have the global numbers
//                    c0 .. c0 + nc - 1; lane l = (c0 + i) mod 64 takes acc = state[l][col], adds the partials of its chunks
//                    i, i + 64, ... of the update in ascending order and stores acc.  A split segment's chunk value is the
//                    class_tree of its eight class sums, as k_fmom_fold joins them.  A thread per (lane, column), coalesced along
//                    the columns; no atomics, nothing sized by the device.
// The rows left over, fewer than 128, go to the tail.  finish runs the tail as the last, short chunk and then
//   k_faccum_finish  a thread per column: the 64 lane partials in registers, for off = 32 .. 1 lane l < off takes p_l + p_(l + off).
// A lane that starts at +0.0 and continues the same additions in the same order over the calls holds what the one-shot fold's lane
// holds: that is the whole argument for equal bits.
#include "staging.hpp"
#include "field_partials.hpp"

using bluest_partials::FChunk;
using bluest_partials::ZChunk;

namespace {

constexpr int BLK = 256;

__global__ __launch_bounds__(BLK) void k_faccum_carry(double *__restrict__ lanes_s, double *__restrict__ lanes_m,
                                                      const double *__restrict__ part_s, const double *__restrict__ part_m, int64_t W,
                                                      int64_t W2, int split, int64_t c0, int64_t nc)
{
    const int64_t i = blockIdx.y, lane = (c0 + i) & (WAVE - 1);
    const int64_t step = split ? CLASSES * W2 : W2;
    for (int64_t col = (int64_t)blockIdx.x * BLK + threadIdx.x; col < W + W2; col += (int64_t)gridDim.x * BLK) {
        if (col < W) {
            double acc = lanes_s[lane * W + col];
            for (int64_t k = i; k < nc; k += WAVE) acc += part_s[k * W + col];
            lanes_s[lane * W + col] = acc;
        } else {
            const int64_t x = col - W;
            double acc = lanes_m[lane * W2 + x];
            for (int64_t k = i; k < nc; k += WAVE) {
                const double *pc = part_m + k * step + x;
                acc += split ? class_tree(pc, (int)W2) : pc[0];
            }
            lanes_m[lane * W2 + x] = acc;
        }
    }
}

// out: [W] sums, then [2 d] zsum | zsq
__global__ __launch_bounds__(BLK) void k_faccum_finish(const double *__restrict__ lanes_s, const double *__restrict__ lanes_m, int64_t W,
                                                       int64_t W2, double *__restrict__ out)
{
    for (int64_t col = (int64_t)blockIdx.x * BLK + threadIdx.x; col < W + W2; col += (int64_t)gridDim.x * BLK) {
        const double *src = col < W ? lanes_s + col : lanes_m + (col - W);
        const int64_t stride = col < W ? W : W2;
        double p[WAVE];
#pragma unroll
        for (int l = 0; l < WAVE; l++) p[l] = src[l * stride];
#pragma unroll
        for (int off = WAVE / 2; off > 0; off >>= 1) {
#pragma unroll
            for (int l = 0; l < off; l++) p[l] += p[l + off];
        }
        out[col] = p[0];
    }
}

unsigned col_blocks(int64_t cols) { return (unsigned)std::min<int64_t>((cols + BLK - 1) / BLK, 1 << 20); }

}  // namespace

struct bluest_field_accum {
    int L = 0;
    int64_t d = 0, W = 0, W2 = 0;           // W2 = 2 d with coefficients, else 0
    bool split = false;
    int sb = 0, lds = 0;
    int64_t per_chunk = 0;                  // doubles a chunk leaves in part_m
    char *fixed = nullptr;                  // lanes_s, lanes_m, first, tail, coef: one allocation
    double *lanes_s = nullptr, *lanes_m = nullptr, *first = nullptr, *tail = nullptr, *coef = nullptr;
    char *scratch = nullptr;                // grow-only
    size_t scratch_bytes = 0, fixed_bytes = 0;
    int64_t count = 0, chunks_done = 0, allocations = 0, sum_launches = 0, moment_launches = 0;
    int tail_rows = 0;
    bool finished = false;
    std::vector<FChunk> ft;                 // the chunk tables of the running call on the host: they must outlive its copies,
    std::vector<ZChunk> zt;                 // which are read when the stream gets to them, up to the call's synchronise
};

namespace {

hipError_t grow(bluest_field_accum *a, size_t bytes)
{
    if (bytes <= a->scratch_bytes) return hipSuccess;
    if (a->scratch) (void)hipFree(a->scratch);
    a->scratch = nullptr;
    a->scratch_bytes = 0;
    const hipError_t e = hipMalloc((void **)&a->scratch, bytes);
    if (e == hipSuccess) {
        a->scratch_bytes = bytes;
        a->allocations++;
    }
    return e;
}

// The chunks of one update (or of finish): nc of them, the first from the tail buffer when `tail_rows` > 0, then `whole` full
// chunks from `src` (device: where they lie; host: through the staging buffer in slabs of whole chunks).  Partials, carry.
int run_chunks(bluest_field_accum *a, int tail_rows, const double *src, int64_t whole, bool device, size_t out_doubles, double **out,
               hipStream_t st)
{
    const int64_t W = a->W, nt = tail_rows > 0 ? 1 : 0, nc = nt + whole;
    const size_t chunk_bytes = (size_t)GCHUNK * W * 8;
    const int64_t slab_chunks = (device || whole == 0) ? 0 : std::min<int64_t>(whole, std::max<int64_t>(1, slab_budget() / (int64_t)chunk_bytes));
    DeviceArena plan;                       // (only its offsets: the block is the handle's scratch)
    const size_t o_ps = plan.take((size_t)nc * W * 8), o_pm = plan.take((size_t)nc * a->per_chunk * 8),
                 o_ft = plan.take((size_t)nc * sizeof(FChunk)), o_zt = plan.take(a->W2 ? (size_t)nc * sizeof(ZChunk) : 0),
                 o_out = plan.take(out_doubles * 8), o_stage = plan.take((size_t)slab_chunks * chunk_bytes);
    HIP_TRY(grow(a, plan.size));
    char *dv = a->scratch;
    double *part_s = (double *)(dv + o_ps), *part_m = (double *)(dv + o_pm);
    const double *stage = (const double *)(dv + o_stage);
    if (out) *out = (double *)(dv + o_out);
    if (nc == 0) return BLUEST_OK;

    std::vector<FChunk> &ft = a->ft;
    std::vector<ZChunk> &zt = a->zt;
    ft.resize((size_t)nc);
    zt.resize(a->W2 ? (size_t)nc : 0);
    for (int64_t i = 0; i < nc; i++) {
        const int64_t k = i - nt;
        const double *rows = i < nt ? a->tail : device ? src + k * GCHUNK * W : stage + (k % slab_chunks) * GCHUNK * W;
        const int32_t n = i < nt ? tail_rows : GCHUNK;
        ft[(size_t)i] = FChunk{rows, i * W, W, n};
        if (a->W2) zt[(size_t)i] = ZChunk{rows, a->first, i * a->per_chunk, n, a->L, 0, a->sb};
    }
    const FChunk *d_ft = (const FChunk *)(dv + o_ft);
    const ZChunk *d_zt = (const ZChunk *)(dv + o_zt);
    HIP_TRY(hipMemcpyAsync(dv + o_ft, ft.data(), (size_t)nc * sizeof(FChunk), hipMemcpyHostToDevice, st));
    if (a->W2) HIP_TRY(hipMemcpyAsync(dv + o_zt, zt.data(), (size_t)nc * sizeof(ZChunk), hipMemcpyHostToDevice, st));

    auto launch = [&](int64_t i0, int64_t n) -> int {
        if (n <= 0) return BLUEST_OK;
        HIP_TRY(bluest_partials::launch_fsum_partial(d_ft + i0, (size_t)n, W, part_s, st));
        a->sum_launches++;
        if (a->W2) {
            HIP_TRY(bluest_partials::launch_fmom_partial(d_zt + i0, (size_t)n, a->split, a->lds, a->d, a->coef, part_m, st));
            a->moment_launches++;
        }
        return BLUEST_OK;
    };
    if (device || whole == 0) {
        const int rc = launch(0, nc); if (rc) return rc;
    } else {
        for (int64_t k0 = 0; k0 < whole; k0 += slab_chunks) {           // in stream order: the next slab's copy waits for the kernels
            const int64_t n = std::min(slab_chunks, whole - k0);
            HIP_TRY(hipMemcpyAsync(dv + o_stage, src + k0 * GCHUNK * W, (size_t)n * chunk_bytes, hipMemcpyHostToDevice, st));
            const int rc = k0 == 0 ? launch(0, nt + n) : launch(nt + k0, n); if (rc) return rc;
        }
    }
    const dim3 grid(col_blocks(W + a->W2), (unsigned)std::min<int64_t>(nc, WAVE));
    hipLaunchKernelGGL(k_faccum_carry, grid, dim3(BLK), 0, st, a->lanes_s, a->lanes_m, (const double *)part_s, (const double *)part_m, W, a->W2,
                       (int)a->split, a->chunks_done, nc);
    HIP_TRY(hipGetLastError());
    a->chunks_done += nc;
    return BLUEST_OK;
}

}  // namespace

extern "C" int bluest_field_accum_create(int L, int64_t d, const double *coef, bluest_field_accum **out, void *stream)
{
    if (!out) return fail(BLUEST_ERR_ARG, "null pointer");
    if (L < 1 || L > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "L=%d out of range (1..%d)", L, BLUEST_MAX_MODELS);
    if (d < 1) return fail(BLUEST_ERR_ARG, "d=%lld: at least one component is needed", (long long)d);
    if ((double)L * (double)d > 2147483647.0) return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 column-components L d");
    if (coef)
        for (int j = 0; j < L; j++)
            if (!std::isfinite(coef[j])) return fail(BLUEST_ERR_ARG, "coef[%d]=%g is not finite", j, coef[j]);
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    bluest_field_accum *a = new bluest_field_accum;
    a->L = L; a->d = d; a->W = (int64_t)L * d; a->W2 = coef ? 2 * d : 0;
    if (coef) {
        a->split = bluest_partials::field_moments_split(L, d);
        a->sb = bluest_partials::field_moments_rows(L, d);
        a->lds = bluest_partials::field_moments_lds(L, d);
        a->per_chunk = a->W2 * (a->split ? CLASSES : 1);
    }
    DeviceArena plan;
    const size_t o_ls = plan.take((size_t)WAVE * a->W * 8), o_lm = plan.take((size_t)WAVE * a->W2 * 8), o_first = plan.take((size_t)a->W * 8),
                 o_tail = plan.take((size_t)GCHUNK * a->W * 8), o_coef = plan.take(coef ? (size_t)L * 8 : 0);
    hipError_t e = hipMalloc((void **)&a->fixed, plan.size);
    if (e == hipSuccess) e = hipMemsetAsync(a->fixed, 0, o_first, st);                  // the lanes start at +0.0
    if (e == hipSuccess && coef) e = hipMemcpyAsync(a->fixed + o_coef, coef, (size_t)L * 8, hipMemcpyHostToDevice, st);
    if (e == hipSuccess) e = hipStreamSynchronize(st);
    if (e != hipSuccess) {
        if (a->fixed) (void)hipFree(a->fixed);
        delete a;
        return fail(BLUEST_ERR_HIP, "bluest_field_accum_create: %s", hipGetErrorString(e));
    }
    a->fixed_bytes = plan.size;
    a->allocations = 1;
    a->lanes_s = (double *)(a->fixed + o_ls); a->lanes_m = (double *)(a->fixed + o_lm); a->first = (double *)(a->fixed + o_first);
    a->tail = (double *)(a->fixed + o_tail); a->coef = (double *)(a->fixed + o_coef);
    *out = a;
    return BLUEST_OK;
}

extern "C" int bluest_field_accum_update(bluest_field_accum *a, int64_t rows, const double *values, void *stream)
{
    if (!a) return fail(BLUEST_ERR_ARG, "null handle");
    if (rows < 0) return fail(BLUEST_ERR_ARG, "rows=%lld is negative", (long long)rows);
    if (rows > 0 && !values) return fail(BLUEST_ERR_ARG, "values is null");
    if (rows > 0 && ((uintptr_t)values & 7)) return fail(BLUEST_ERR_ARG, "values is not 8-byte aligned");
    if ((double)(rows / GCHUNK + 2) * (double)((a->d + WAVE - 1) / WAVE) * CLASSES > 2147483647.0)
        return fail(BLUEST_ERR_ARG, "more than 2^31 - 1 (chunk, block of %d components, class) workgroups in one update", WAVE);
    if (a->finished) return fail(BLUEST_ERR_STATE, "the accumulator is finished");
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    if (rows > 0) {
        const bool device = on_device(values);
        const hipMemcpyKind kind = device ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice;
        const int64_t W = a->W;
        if (a->count == 0) HIP_TRY(hipMemcpyAsync(a->first, values, (size_t)W * 8, kind, st));
        const double *src = values;
        int64_t left = rows;
        int t = a->tail_rows;
        if (t > 0) {                                                    // the straddling chunk is completed inside the tail buffer
            const int64_t need = std::min<int64_t>(GCHUNK - t, left);
            HIP_TRY(hipMemcpyAsync(a->tail + (int64_t)t * W, src, (size_t)need * W * 8, kind, st));
            t += (int)need; src += need * W; left -= need;
        }
        const int64_t whole = left / GCHUNK, rest = left % GCHUNK;
        const bool full_tail = t == GCHUNK;
        if (full_tail || whole > 0) {
            rc = run_chunks(a, full_tail ? GCHUNK : 0, src, whole, device, 0, nullptr, st); if (rc) return rc;
        }
        if (full_tail) t = 0;
        if (rest > 0) {                                                 // (only with an empty tail; behind the kernels that read it)
            HIP_TRY(hipMemcpyAsync(a->tail, src + whole * GCHUNK * W, (size_t)rest * W * 8, kind, st));
            t = (int)rest;
        }
        a->tail_rows = t;
        a->count += rows;
    }
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

extern "C" int bluest_field_accum_finish(bluest_field_accum *a, int64_t *count, double *sums, double *zsum, double *zsq, void *stream)
{
    if (!a || !count || !sums) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((zsum == nullptr) != (zsq == nullptr)) return fail(BLUEST_ERR_ARG, "zsum and zsq must both be given or both be null");
    if ((zsum != nullptr) != (a->W2 != 0)) return fail(BLUEST_ERR_ARG, "zsum and zsq go with the coefficients given at creation, and only with them");
    if (a->finished) return fail(BLUEST_ERR_STATE, "the accumulator is finished");
    int rc = require_gpu(); if (rc) return rc;
    hipStream_t st = (hipStream_t)stream;
    double *d_out = nullptr;
    rc = run_chunks(a, a->tail_rows, nullptr, 0, true, (size_t)(a->W + a->W2), &d_out, st); if (rc) return rc;
    a->tail_rows = 0;
    hipLaunchKernelGGL(k_faccum_finish, dim3(col_blocks(a->W + a->W2)), dim3(BLK), 0, st, (const double *)a->lanes_s, (const double *)a->lanes_m,
                       a->W, a->W2, d_out);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(sums, d_out, (size_t)a->W * 8, hipMemcpyDeviceToHost, st));
    if (zsum) {
        HIP_TRY(hipMemcpyAsync(zsum, d_out + a->W, (size_t)a->d * 8, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipMemcpyAsync(zsq, d_out + a->W + a->d, (size_t)a->d * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    *count = a->count;
    a->finished = true;
    return BLUEST_OK;
}

extern "C" int bluest_field_accum_info(const bluest_field_accum *a, int64_t *info)
{
    if (!a || !info) return fail(BLUEST_ERR_ARG, "null pointer");
    info[0] = a->count; info[1] = a->chunks_done; info[2] = a->tail_rows; info[3] = a->allocations;
    info[4] = a->sum_launches; info[5] = a->moment_launches; info[6] = (int64_t)(a->fixed_bytes + a->scratch_bytes); info[7] = a->finished;
    return BLUEST_OK;
}

extern "C" int bluest_field_accum_destroy(bluest_field_accum *a)
{
    if (!a) return BLUEST_OK;
    if (a->scratch) (void)hipFree(a->scratch);
    if (a->fixed) (void)hipFree(a->fixed);
    delete a;
    return BLUEST_OK;
}

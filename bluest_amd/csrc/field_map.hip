// field_map.hip -- Part 18 of include/bluest_hip.h: sparse maps B_l (q x d_l) that take the models of a field output from their
// own meshes into a space they share, out[s, l, :] = B_l y_l[s, :], so that everything downstream (Parts 12 and 15 to 17) sees
// one array [N, L, q].  An operator is checked, laid out (field_op_layout.hpp) and uploaded ONCE, when its handle is made.
//
// The pass is bound by memory: 8 N (sum of d_l + L q) bytes of values per call against operators that stay in L2.
//   k_fm_short   rows of at most BLUEST_FIELD_MAP_STRIP entries.  A wavefront takes a slice of 64 rows -- lane = row -- and a block
//                of SB = 8 samples whose chains it keeps in registers: an operator entry is read once per block of samples, the
//                64 lanes read 64 consecutive slots of the sliced ELL, and every store is 64 consecutive doubles of out[s, l, :].
//                The gathers y[s, indices[k]] of neighbouring rows land on neighbouring columns for a mesh operator and are left
//                to the caches.  The loop runs to the slice's width under `k < len`: a padded slot is never executed.
//   k_fm_long    rows of more than a strip.  A wavefront takes a bundle of up to 8 long rows with the same column sequence
//                (the rows of a dense functional; otherwise one row) and 64 samples, lane = sample, and walks the strips in
//                ascending order: the values are gathered ONCE per bundle, tile by tile, into LDS along the entries and read back
//                with a lane per sample; the chain of a strip and the sum of the strips stay in the lane.
//   k_fm_copy    an identity entry: the value's 64 bits.
// One launch per model and kernel.  Which kernel a row gets follows from its length only, so no bit depends on it.  No atomics,
// nothing sized by the number of compute units.
// Staging: host values and a host `out` pass through the call's one arena in runs of whole samples under the budget of
// bluest_group_sums_slab; an output element depends on one sample, so nothing is folded.  Device memory is used where it lies.
#include "staging.hpp"
#include "field_op_layout.hpp"

struct bluest_field_op {
    uint32_t magic;
    int64_t q, d, nnz, nslices, nlong, nbundles;
    char *base;                         // the one device allocation
    const int32_t *len, *ell_idx, *long_row, *long_idx, *bundle_at;
    const int64_t *slice_at, *long_at;
    const double *ell_val, *long_val;
};

namespace {

constexpr uint32_t FM_MAGIC = 0x464d4f50u;
constexpr int BLK = 256, WAVES = BLK / WAVE;
constexpr int SB = 8;                               // samples a wavefront keeps in registers
constexpr int64_t STRIP = BLUEST_FIELD_MAP_STRIP;
constexpr int64_t RUN_MAX = 65535LL * WAVES;        // samples per run: the sample blocks of a launch fit grid.y
constexpr int LBLK = 128, LTILE = 32;               // k_fm_long: threads per workgroup; entries per LDS tile (half a wavefront)
static_assert(2 * LTILE == WAVE, "a wavefront gathers LTILE entries of two samples at a time");
static_assert(FM_SLICE == WAVE, "lane = row");
static_assert((STRIP & (STRIP - 1)) == 0, "the strip is a power of two");

struct FmOp {                                       // what a kernel reads of an operator
    const int32_t *len, *ell_idx, *long_row, *long_idx, *bundle_at;
    const int64_t *slice_at, *long_at;
    const double *ell_val, *long_val;
    int64_t q, d, nslices;
};

// grid (slices / 4 rounded up, sample blocks); y: sample 0 of the run [ns][d]; out: (sample 0 of the run, this model, row 0),
// `stride` doubles from sample to sample
__global__ __launch_bounds__(BLK) void k_fm_short(FmOp op, const double *__restrict__ y, int64_t ns, double *__restrict__ out, int64_t stride)
{
    const int lane = threadIdx.x & (WAVE - 1);
    const int64_t slice = (int64_t)blockIdx.x * WAVES + (threadIdx.x >> 6);
    if (slice >= op.nslices) return;
    const int64_t r = slice * WAVE + lane, s0 = (int64_t)blockIdx.y * SB;
    const int n = op.len[r];                                           // padded to whole slices
    const int64_t at = op.slice_at[slice];
    const int width = (int)((op.slice_at[slice + 1] - at) >> 6);
    const int32_t *idx = op.ell_idx + at + lane;
    const double *val = op.ell_val + at + lane;
    const double *ys[SB];
#pragma unroll
    for (int s = 0; s < SB; s++) ys[s] = y + min(s0 + s, ns - 1) * op.d;     // past the run: the last sample again, never stored
    double p[SB];
#pragma unroll
    for (int s = 0; s < SB; s++) p[s] = 0.0;
    for (int k = 0; k < width; k++) {
        if (k < n) {
            const int32_t c = idx[(int64_t)k * WAVE];
            const double a = val[(int64_t)k * WAVE];
#pragma unroll
            for (int s = 0; s < SB; s++) p[s] = fma(a, ys[s][c], p[s]);
        }
    }
    if (n < 0) return;                                                 // a long row, or past q
#pragma unroll
    for (int s = 0; s < SB; s++)
        if (s0 + s < ns) out[(s0 + s) * stride + r] = p[s];
}

// grid (bundles of long rows, blocks of 64 samples / 2 rounded up), LBLK = 2 wavefronts.  A wavefront takes a bundle -- up to
// FM_BUNDLE long rows with the same column sequence, mostly one -- and 64 samples, lane = sample, and walks the strips one after
// the other.  Per sub-tile of LTILE entries the values y[s, idx[k]] are gathered into the wavefront's own LDS tile along k -- a
// half-wave reads LTILE entries of one sample: 256 consecutive bytes where the columns are consecutive, as in a dense functional --
// and read back with a lane per sample (row stride LTILE + 1: conflict-free); the coefficients are wave-uniform.  A strip's chain
// and the sum of the strips stay in the lane: the order is that of Part 18 as it stands.
__global__ __launch_bounds__(LBLK) void k_fm_long(FmOp op, const double *__restrict__ y, int64_t ns, double *__restrict__ out, int64_t stride)
{
    __shared__ double tiles[LBLK / WAVE][WAVE * (LTILE + 1)];
    const int lane = threadIdx.x & (WAVE - 1), w = threadIdx.x >> 6;
    const int64_t s0 = ((int64_t)blockIdx.y * (LBLK / WAVE) + w) * WAVE;
    if (s0 >= ns) return;                                              // the whole wavefront; the kernel has no workgroup barrier
    double *G = tiles[w];
    const int j0 = op.bundle_at[blockIdx.x], nr = op.bundle_at[blockIdx.x + 1] - j0;
    const int64_t a0 = op.long_at[j0], n = op.long_at[j0 + 1] - a0;   // every row of the bundle has n entries and row j0's columns
    const int e = lane & (LTILE - 1), half = lane >> 5;
    double total[FM_BUNDLE], p[FM_BUNDLE];
#pragma unroll
    for (int r = 0; r < FM_BUNDLE; r++) total[r] = 0.0;
    for (int64_t kb = 0; kb < n; kb += STRIP) {
        const int64_t ke = min(kb + STRIP, n);
#pragma unroll
        for (int r = 0; r < FM_BUNDLE; r++) p[r] = 0.0;
        for (int64_t k0 = kb; k0 < ke; k0 += LTILE) {
            const int ne = (int)min((int64_t)LTILE, ke - k0);
            wave_lds_sync();                                           // the reads of the last tile are done
            if (e < ne) {
                const int64_t c = op.long_idx[a0 + k0 + e];
#pragma unroll 8
                for (int i = 0; i < WAVE / 2; i++) {
                    const int s = 2 * i + half;
                    G[s * (LTILE + 1) + e] = y[min(s0 + s, ns - 1) * op.d + c];      // past the run: the last sample again, never stored
                }
            }
            wave_lds_sync();
            for (int t = 0; t < ne; t++) {
                const double g = G[lane * (LTILE + 1) + t];
#pragma unroll
                for (int r = 0; r < FM_BUNDLE; r++)
                    if (r < nr) p[r] = fma(op.long_val[a0 + (int64_t)r * n + k0 + t], g, p[r]);
            }
        }
#pragma unroll
        for (int r = 0; r < FM_BUNDLE; r++) total[r] = total[r] + p[r];
    }
    if (s0 + lane < ns) {
#pragma unroll
        for (int r = 0; r < FM_BUNDLE; r++)
            if (r < nr) out[(s0 + lane) * stride + op.long_row[j0 + r]] = total[r];
    }
}

// grid (q / 256 rounded up, samples up to 65535): an identity entry, bit for bit
__global__ __launch_bounds__(BLK) void k_fm_copy(const unsigned long long *__restrict__ y, int64_t ns, int64_t q, unsigned long long *__restrict__ out,
                                                 int64_t stride)
{
    const int64_t r = (int64_t)blockIdx.x * BLK + threadIdx.x;
    if (r >= q) return;
    for (int64_t s = blockIdx.y; s < ns; s += gridDim.y) out[s * stride + r] = y[s * q + r];
}

template <class T>
size_t put(std::vector<char> &blob, const std::vector<T> &v)
{
    const size_t at = blob.size(), bytes = v.size() * sizeof(T);
    blob.resize(at + ((std::max<size_t>(bytes, 1) + 255) & ~(size_t)255), 0);
    if (bytes) memcpy(blob.data() + at, v.data(), bytes);
    return at;
}

}  // namespace

extern "C" int bluest_field_op_create(int64_t q, int64_t d, const int64_t *indptr, const int32_t *indices, const double *data,
                                      bluest_field_op_t *op)
{
    if (!op) return fail(BLUEST_ERR_ARG, "op is null");
    const std::string why = check_field_csr(q, d, indptr, indices, data);
    if (!why.empty()) return fail(BLUEST_ERR_ARG, "%s", why.c_str());
    int rc = require_gpu(); if (rc) return rc;
    const FieldOpLayout lay = layout_field_csr(q, d, indptr, indices, data, STRIP);
    std::vector<char> blob;
    const size_t o_len = put(blob, lay.len), o_at = put(blob, lay.slice_at), o_ei = put(blob, lay.ell_idx), o_ev = put(blob, lay.ell_val),
                 o_lr = put(blob, lay.long_row), o_la = put(blob, lay.long_at), o_li = put(blob, lay.long_idx), o_lv = put(blob, lay.long_val),
                 o_ba = put(blob, lay.bundle_at);
    char *base = nullptr;
    HIP_TRY(hipMalloc((void **)&base, blob.size()));
    const hipError_t e = hipMemcpy(base, blob.data(), blob.size(), hipMemcpyHostToDevice);
    if (e != hipSuccess) {
        (void)hipFree(base);
        return fail(BLUEST_ERR_HIP, "uploading the operator failed: %s", hipGetErrorString(e));
    }
    bluest_field_op *h = new bluest_field_op;
    h->magic = FM_MAGIC;
    h->q = q; h->d = d; h->nnz = lay.nnz; h->nslices = lay.nslices; h->nlong = (int64_t)lay.long_row.size();
    h->base = base;
    h->len = (const int32_t *)(base + o_len); h->slice_at = (const int64_t *)(base + o_at);
    h->ell_idx = (const int32_t *)(base + o_ei); h->ell_val = (const double *)(base + o_ev);
    h->long_row = (const int32_t *)(base + o_lr); h->long_at = (const int64_t *)(base + o_la);
    h->long_idx = (const int32_t *)(base + o_li); h->long_val = (const double *)(base + o_lv);
    h->bundle_at = (const int32_t *)(base + o_ba);
    h->nbundles = (int64_t)lay.bundle_at.size() - 1;
    *op = h;
    return BLUEST_OK;
}

extern "C" int bluest_field_op_shape(bluest_field_op_t op, int64_t *q, int64_t *d, int64_t *nnz)
{
    if (!op || op->magic != FM_MAGIC) return fail(BLUEST_ERR_ARG, "op is null or not a live operator");
    if (q) *q = op->q;
    if (d) *d = op->d;
    if (nnz) *nnz = op->nnz;
    return BLUEST_OK;
}

extern "C" int bluest_field_op_destroy(bluest_field_op_t op)
{
    if (!op || op->magic != FM_MAGIC) return fail(BLUEST_ERR_ARG, "op is null or not a live operator");
    op->magic = 0;
    const hipError_t e = hipFree(op->base);
    delete op;
    if (e != hipSuccess) return fail(BLUEST_ERR_HIP, "hipFree failed: %s", hipGetErrorString(e));
    return BLUEST_OK;
}

extern "C" int bluest_field_map(int64_t N, int L, int64_t q, const bluest_field_op_t *ops, const double *const *values, double *out,
                                void *stream)
{
    if (L < 1 || L > BLUEST_MAX_MODELS) return fail(BLUEST_ERR_ARG, "L=%d out of range (1..%d)", L, BLUEST_MAX_MODELS);
    if (N < 0) return fail(BLUEST_ERR_ARG, "N=%lld is negative", (long long)N);
    if (q < 1) return fail(BLUEST_ERR_ARG, "q=%lld: at least one row is needed", (long long)q);
    if (!values) return fail(BLUEST_ERR_ARG, "values is null");
    int64_t width[BLUEST_MAX_MODELS];
    for (int l = 0; l < L; l++) {
        const bluest_field_op *op = ops ? ops[l] : nullptr;
        if (op && op->magic != FM_MAGIC) return fail(BLUEST_ERR_ARG, "ops[%d] is not a live operator", l);
        if (op && op->q != q) return fail(BLUEST_ERR_ARG, "ops[%d] has %lld rows, the call q=%lld", l, (long long)op->q, (long long)q);
        width[l] = op ? op->d : q;                                     // an identity entry: d_l == q
        if (N > 0 && !values[l]) return fail(BLUEST_ERR_ARG, "values[%d] is null", l);
        if ((uintptr_t)values[l] & 7) return fail(BLUEST_ERR_ARG, "values[%d] is not 8-byte aligned", l);
    }
    if (N > 0 && !out) return fail(BLUEST_ERR_ARG, "out is null");
    if ((uintptr_t)out & 7) return fail(BLUEST_ERR_ARG, "out is not 8-byte aligned");
    int rc = require_gpu(); if (rc) return rc;
    if (N == 0) return BLUEST_OK;
    hipStream_t st = (hipStream_t)stream;

    // runs of whole samples: what the staging budget allows of the host arrays, at least one sample
    const int64_t stride = (int64_t)L * q;
    bool host[BLUEST_MAX_MODELS];
    const bool out_host = !on_device(out);
    int64_t sample_bytes = out_host ? stride * 8 : 0;
    for (int l = 0; l < L; l++) {
        host[l] = !on_device(values[l]);
        if (host[l]) sample_bytes += width[l] * 8;
    }
    int64_t run = std::min(N, RUN_MAX);
    if (sample_bytes > 0) run = std::min(run, std::max<int64_t>(1, slab_budget() / sample_bytes));
    DeviceArena arena;
    size_t o_in[BLUEST_MAX_MODELS];
    for (int l = 0; l < L; l++) o_in[l] = host[l] ? arena.take((size_t)run * width[l] * 8) : 0;
    const size_t o_out = out_host ? arena.take((size_t)run * stride * 8) : 0;
    if (arena.size > 0) HIP_TRY(arena.alloc());

    for (int64_t s0 = 0; s0 < N; s0 += run) {
        const int64_t ns = std::min(run, N - s0);
        double *dst = out_host ? (double *)(arena.base + o_out) : out + s0 * stride;
        const unsigned sblocks = (unsigned)((ns - 1) / SB + 1);
        for (int l = 0; l < L; l++) {
            const double *src = values[l] + s0 * width[l];
            if (host[l]) {                                             // in stream order: the copy waits for the kernels of the last run
                HIP_TRY(hipMemcpyAsync(arena.base + o_in[l], src, (size_t)ns * width[l] * 8, hipMemcpyHostToDevice, st));
                src = (const double *)(arena.base + o_in[l]);
            }
            const bluest_field_op *h = ops ? ops[l] : nullptr;
            if (!h) {
                const dim3 grid((unsigned)((q - 1) / BLK + 1), (unsigned)std::min<int64_t>(ns, 65535));
                hipLaunchKernelGGL(k_fm_copy, grid, dim3(BLK), 0, st, (const unsigned long long *)src, ns, q, (unsigned long long *)(dst + (int64_t)l * q),
                                   stride);
                HIP_TRY(hipGetLastError());
                continue;
            }
            const FmOp op{h->len, h->ell_idx, h->long_row, h->long_idx, h->bundle_at, h->slice_at, h->long_at, h->ell_val, h->long_val, h->q, h->d,
                          h->nslices};
            hipLaunchKernelGGL(k_fm_short, dim3((unsigned)((h->nslices - 1) / WAVES + 1), sblocks), dim3(BLK), 0, st, op, src, ns,
                               dst + (int64_t)l * q, stride);
            HIP_TRY(hipGetLastError());
            if (h->nlong > 0) {
                const unsigned lblocks = (unsigned)((ns - 1) / (WAVE * (LBLK / WAVE)) + 1);
                hipLaunchKernelGGL(k_fm_long, dim3((unsigned)h->nbundles, lblocks), dim3(LBLK), 0, st, op, src, ns, dst + (int64_t)l * q, stride);
                HIP_TRY(hipGetLastError());
            }
        }
        if (out_host) HIP_TRY(hipMemcpyAsync(out + s0 * stride, dst, (size_t)ns * stride * 8, hipMemcpyDeviceToHost, st));
    }
    HIP_TRY(hipStreamSynchronize(st));
    return BLUEST_OK;
}

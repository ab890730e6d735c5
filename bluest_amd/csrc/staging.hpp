// staging.hpp -- what the sample-sum entry points (pilot.hip, pilot4.hip, gsums.hip, fields.hip, moments.hip, field_moments.hip,
// field_cov.hip, field_pilot.hip, field_map.hip) share: telling a host pointer from a device pointer, the one device allocation of a call, the pair -> thread map of the pilot
// statistics, and the mechanism of the four calls over many ragged segments (bluest_group_sums, bluest_field_sums,
// bluest_group_moments, bluest_field_weighted_moments):
//   - the checks of a segment's arguments (check_segment);
//   - the chunk: GCHUNK consecutive rows of a segment, summed in eight classes of sixteen rows that join in a fixed tree
//     (class_tree; Part 11 of include/bluest_hip.h);
//   - the slabs: device segments are read where they lie, host segments are cut into pieces of whole chunks that share one
//     staging buffer slab by slab (slab_plan.hpp; the budget is that of bluest_group_sums_slab, slab_budget);
//   - the chunk table: the chunks of every launch -- group 0 the device segments, group 1 + k slab k, inside a group one list per
//     kernel shape -- lie together in one table that is uploaded once, before anything is copied (ChunkLists);
//   - the slab loop: group 0, then per slab its copies and its launches in stream order (run_slabs).
// The chunks' partial sums all land in one buffer that a single fold reads, so a slab boundary never shows in a result.
#pragma once
#include "common.hpp"
#include "slab_plan.hpp"

namespace {

constexpr int GCHUNK = BLUEST_GSUM_CHUNK;
constexpr int CLASSES = 8, CLASS_ROWS = GCHUNK / CLASSES;
static_assert(CLASSES * CLASS_ROWS == GCHUNK && CLASS_ROWS == 16, "the row classes tile the chunk");

// the fixed tree of Part 11 over eight class sums, `stride` doubles apart or in registers
__device__ __forceinline__ double class_tree(const double *c, int stride)
{
    return ((c[0] + c[stride]) + (c[2 * stride] + c[3 * stride])) + ((c[4 * stride] + c[5 * stride]) + (c[6 * stride] + c[7 * stride]));
}
__device__ __forceinline__ double class_tree(const double (&q)[CLASSES])
{
    return ((q[0] + q[1]) + (q[2] + q[3])) + ((q[4] + q[5]) + (q[6] + q[7]));
}

inline bool on_device(const void *p)
{
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
}

// the staging budget of a call (bluest_group_sums_slab)
inline int64_t slab_budget()
{
    int64_t bytes = BLUEST_GSUM_SLAB_BYTES;
    (void)bluest_group_sums_slab(0, &bytes);
    return bytes;
}

// segment s of a ragged call; repeat_of (null: the call has no repeats) must lie in 0..R-1 and not decrease
inline int check_segment(int64_t s, const int64_t *counts, const int32_t *sizes, const double *const *values,
                         const int64_t *repeat_of = nullptr, int R = 0)
{
    if (sizes[s] < 1 || sizes[s] > BLUEST_MAX_MODELS)
        return fail(BLUEST_ERR_ARG, "sizes[%lld]=%d out of range (1..%d)", (long long)s, sizes[s], BLUEST_MAX_MODELS);
    if (counts[s] < 0) return fail(BLUEST_ERR_ARG, "counts[%lld]=%lld is negative", (long long)s, (long long)counts[s]);
    if (counts[s] > 0 && !values[s]) return fail(BLUEST_ERR_ARG, "values[%lld] is null", (long long)s);
    if (counts[s] > 0 && ((uintptr_t)values[s] & 7)) return fail(BLUEST_ERR_ARG, "values[%lld] is not 8-byte aligned", (long long)s);
    if (repeat_of) {
        if (repeat_of[s] < 0 || repeat_of[s] >= R)
            return fail(BLUEST_ERR_ARG, "repeat_of[%lld]=%lld out of range (0..%d)", (long long)s, (long long)repeat_of[s], R - 1);
        if (s > 0 && repeat_of[s] < repeat_of[s - 1]) return fail(BLUEST_ERR_ARG, "repeat_of decreases at segment %lld", (long long)s);
    }
    return BLUEST_OK;
}

// The one device allocation of a call: take() hands out offsets, 256-byte aligned, alloc() makes the block they lie in, and the
// block goes when the arena does.
struct DeviceArena {
    char *base = nullptr;
    size_t size = 0;
    DeviceArena() = default;
    DeviceArena(const DeviceArena &) = delete;
    DeviceArena &operator=(const DeviceArena &) = delete;
    ~DeviceArena() { if (base) (void)hipFree(base); }
    size_t take(size_t bytes) { const size_t o = size; size += (bytes + 255) & ~(size_t)255; return o; }
    hipError_t alloc() { return hipMalloc((void **)&base, size); }
};

// The chunks of a call, list (launch group g, key) by list: add() takes them in any order, flatten() lays the lists end to end
// in `table`, list (g, key) at [begin(g, key), end(g, key)).  The order inside a list is the order the chunks were added in.
// Chunks that arrive list after list, as those of a call with one key do, are in place already and are not moved again.
template <class Chunk>
struct ChunkLists {
    size_t keys, expected;              // `expected`: the chunks the call counted when it checked its arguments
    std::vector<Chunk> table;
    struct Run { size_t list, at; };    // chunks added one after the other to the same list: from table[at] to the next run
    std::vector<Run> runs;
    std::vector<size_t> list0;
    ChunkLists(size_t groups, size_t keys_, int64_t expected_) : keys(keys_), expected((size_t)expected_), list0(groups * keys_ + 1, 0)
    {
        table.reserve(expected);
    }
    void add(size_t g, size_t key, const Chunk &c)
    {
        const size_t list = g * keys + key;
        if (runs.empty() || runs.back().list != list) runs.push_back(Run{list, table.size()});
        table.push_back(c);
    }
    size_t begin(size_t g, size_t key = 0) const { return list0[g * keys + key]; }
    size_t end(size_t g, size_t key = 0) const { return list0[g * keys + key + 1]; }
    int flatten()
    {
        if (table.size() != expected) return fail(BLUEST_ERR_HIP, "internal: %zu chunks tabled, %lld expected", table.size(), (long long)expected);
        bool sorted = true;
        for (size_t r = 0; r < runs.size(); r++) {
            list0[runs[r].list + 1] += (r + 1 < runs.size() ? runs[r + 1].at : table.size()) - runs[r].at;
            sorted = sorted && (r == 0 || runs[r - 1].list < runs[r].list);
        }
        for (size_t i = 1; i < list0.size(); i++) list0[i] += list0[i - 1];
        if (!sorted) {                      // run by run to its list's place, the runs of a list in the order they came in
            std::vector<Chunk> ordered(table.size());
            std::vector<size_t> next(list0.begin(), list0.end() - 1);
            for (size_t r = 0; r < runs.size(); r++) {
                const size_t n = (r + 1 < runs.size() ? runs[r + 1].at : table.size()) - runs[r].at;
                std::copy(table.begin() + runs[r].at, table.begin() + runs[r].at + n, ordered.begin() + next[runs[r].list]);
                next[runs[r].list] += n;
            }
            table.swap(ordered);
        }
        return BLUEST_OK;
    }
};

// rows [first, first + rows) of the host array src = [planes][N][row doubles] to dst as [planes][rows][row doubles]: one copy
// where the rows lie together (one plane, or all N rows), else one per plane
inline int copy_piece(char *dst, const double *src, int planes, int64_t first, int64_t rows, int64_t row, int64_t N, hipStream_t st)
{
    if (planes == 1 || rows == N) {
        HIP_TRY(hipMemcpyAsync(dst, src + first * row, (size_t)planes * rows * row * 8, hipMemcpyHostToDevice, st));
    } else {
        for (int o = 0; o < planes; o++)
            HIP_TRY(hipMemcpyAsync(dst + (size_t)o * rows * row * 8, src + ((int64_t)o * N + first) * row, (size_t)rows * row * 8,
                                   hipMemcpyHostToDevice, st));
    }
    return BLUEST_OK;
}

// The slab loop: launch(0) for the device segments, then slab by slab the copies of its pieces into `stage` and launch(1 + slab),
// all on `st`: in stream order, so the copies of the next slab wait for the kernels that read this one.  row_bytes as given to
// plan_slabs, `planes` of equal size in every row; launch(g) starts the kernels of group g and returns a hipError_t.
template <class Launch>
int run_slabs(const SlabPlan &plan, char *stage, const double *const *values, const int64_t *counts, const size_t *row_bytes, int planes,
              Launch launch, hipStream_t st)
{
    HIP_TRY(launch((size_t)0));
    for (size_t p = 0; p < plan.pieces.size();) {
        const int slab = plan.pieces[p].slab;
        for (; p < plan.pieces.size() && plan.pieces[p].slab == slab; p++) {
            const Piece &pc = plan.pieces[p];
            const int rc = copy_piece(stage + pc.at, values[pc.seg], planes, pc.first, pc.rows, (int64_t)(row_bytes[pc.seg] / 8 / planes),
                                      counts[pc.seg], st);
            if (rc) return rc;
        }
        HIP_TRY(launch(1 + (size_t)slab));
    }
    return BLUEST_OK;
}

// The pair -> thread map.  All threads read the SAME sample row at a time, so what decides LDS bank conflicts is the set of
// columns a 32-lane half reads with one ds_read_b64: the bank of column i is 2i mod 64, i.e. two columns collide when they differ
// by 32, and equal columns broadcast.  Pairs are therefore numbered along WRAPPED diagonals, q = d L + i -> {i, (i + d) mod L},
// d = 0..ceil(L/2)-1 with L entries each, plus half a diagonal d = L/2 when L is even (L (L+1) / 2 pairs in all).  32 consecutive
// lanes inside one diagonal read 32 consecutive columns i and 32 consecutive columns (i + d) mod L: conflict-free at any L <= 64.
// At L = 64 every half-wave lies inside one diagonal; at other L a half-wave that straddles two diagonals can see a two-way
// conflict on a few columns.  A row-major triangle (fixed i, running j) would instead broadcast i and be fine too, but its rows
// have different lengths, so the half-waves straddle rows almost always; the wrapped diagonals all have length L.
__host__ __device__ inline int n_pairs(int L) { return L * ((L + 1) / 2) + ((L & 1) ? 0 : L / 2); }

__host__ __device__ __forceinline__ void pair_of(int q, int L, int &lo, int &hi)
{
    const int d = q / L, i = q - d * L;
    int j = i + d;
    if (j >= L) j -= L;
    lo = i < j ? i : j;
    hi = i < j ? j : i;
}

// the inverse for i < j: the wrapped-diagonal number of the pair {i, j}
inline int pair_number(int i, int j, int L)
{
    const int d = j - i;
    if (2 * d < L || (2 * d == L)) return d * L + i;        // {i, i + d}; the half diagonal holds i = 0..L/2-1, and i < L/2 here
    return (L - d) * L + j;                                 // {j, (j + L - d) mod L = i}
}

}  // namespace

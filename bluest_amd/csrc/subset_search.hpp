// subset_search.hpp -- what the two model-subset searches (mfmc.hip, mlmc.hip) share: an argmin of (objective, subset bitmask)
// under "smaller objective, then earlier in the reference's enumeration order", and the host loop that rounds only the subsets
// whose lower bound can still win, in windows of increasing lower bound.  Everything is templated on the order predicate
//   struct Order { static __device__ bool before(uint32_t a, uint32_t b); };      // a is enumerated before b (a != b)
// which each unit defines in its own anonymous namespace, so the two instantiations never meet at link time.
#pragma once
#include "common.hpp"

namespace subset_search {

constexpr int BLK = 256;
constexpr int64_t CAND_CAP = 1 << 16;                      // subsets rounded per window
// Counting scans the window loop may spend between two windows that round a subset.  A window that rounds something consumes
// subsets, and there are at most 2^30; a window that comes out empty (the halving overshot below the next lower bound v) at
// least halves the distance from lo to v, and the next one needs one more halving to get there.  From hi - lo down to the
// spacing of doubles at v that is E <= log2((hi - lo) / v) + 53 empty windows of 1, 2, ..., E halvings, E^2/2 scans in all.
// Lower and upper bounds of one problem are sample costs or errors of the same models: a range of 2^30 between them gives
// E <= 83 and fewer than 3500 scans.  Only lower bounds of exactly zero (more than CAND_CAP subsets at LB = 0, lo = -1 halving
// towards them for 1074 windows, some 5e5 scans) need more, and they end in the same message either way.
constexpr int MAX_IDLE_SCANS = 4096;

template <class Order>
__device__ __forceinline__ bool better(double fa, uint32_t ma, double fb, uint32_t mb)
{
    return fa < fb || (fa == fb && fa < INFINITY && Order::before(ma, mb));
}

__device__ __forceinline__ void atomic_min_pos(double *addr, double v)
{   // non-negative doubles order like their bit patterns
    atomicMin((unsigned long long *)addr, (unsigned long long)__double_as_longlong(v));
}
__device__ __forceinline__ void atomic_max_pos(double *addr, double v)
{
    atomicMax((unsigned long long *)addr, (unsigned long long)__double_as_longlong(v));
}

// block-wide argmin of (f, mask) under better(); result valid in thread 0
template <class Order>
__device__ void block_best(double &f, uint32_t &m, double *redf, uint32_t *redm, int tid)
{
    for (int off = 32; off > 0; off >>= 1) {
        const double of = __shfl_xor(f, off, WAVE);
        const uint32_t om = __shfl_xor(m, off, WAVE);
        if (better<Order>(of, om, f, m)) { f = of; m = om; }
    }
    if ((tid & 63) == 0) { redf[tid >> 6] = f; redm[tid >> 6] = m; }
    __syncthreads();
    if (tid == 0)
        for (int k = 1; k < (int)(blockDim.x >> 6); k++)
            if (better<Order>(redf[k], redm[k], f, m)) { f = redf[k]; m = redm[k]; }
    __syncthreads();
}

// best of `count` (obj, mask[, combos]) records merged into best[0] (obj) / bmask[0] / bcombo[n_out]
template <class Order>
__global__ __launch_bounds__(BLK) void k_pick(int64_t count, const double *f, const uint32_t *m, const uint32_t *idxmask,
                                              const uint32_t *combo, int n_out, double *best, uint32_t *bmask, uint32_t *bcombo)
{
    __shared__ double redf[BLK / WAVE];
    __shared__ uint32_t redm[BLK / WAVE];
    __shared__ int64_t redk[BLK / WAVE];
    const int tid = threadIdx.x;
    double bf = INFINITY;
    uint32_t bm = 0xffffffffu;
    int64_t bk = -1;
    for (int64_t k = tid; k < count; k += BLK) {
        const uint32_t mk = idxmask ? idxmask[k] : m[k];
        if (better<Order>(f[k], mk, bf, bm)) { bf = f[k]; bm = mk; bk = k; }
    }
    for (int off = 32; off > 0; off >>= 1) {
        const double of = __shfl_xor(bf, off, WAVE);
        const uint32_t om = __shfl_xor(bm, off, WAVE);
        const int64_t ok = __shfl_xor(bk, off, WAVE);
        if (better<Order>(of, om, bf, bm)) { bf = of; bm = om; bk = ok; }
    }
    if ((tid & 63) == 0) { redf[tid >> 6] = bf; redm[tid >> 6] = bm; redk[tid >> 6] = bk; }
    __syncthreads();
    if (tid == 0) {
        for (int k = 1; k < BLK / WAVE; k++)
            if (better<Order>(redf[k], redm[k], bf, bm)) { bf = redf[k]; bm = redm[k]; bk = redk[k]; }
        if (bk >= 0 && better<Order>(bf, bm, best[0], bmask[0])) {
            best[0] = bf;
            bmask[0] = bm;
            if (combo) for (int n = 0; n < n_out; n++) bcombo[n] = combo[bk * n_out + n];
        }
    }
}

// The host loop of the integer mode: windows lo < LB <= T of increasing LB, at most CAND_CAP subsets each, the upper end
// tightened by the best objective so far.  U = the smallest upper bound, LBmax = the largest finite lower bound (from the
// unit's first scan); `what` names a subset in messages ("clique", "group").
//   count_in(collect, lo, T, &c): scan, count the subsets with lo < LB <= T into c (collect: also list the first CAND_CAP)
//   round_them(c, &best):         round the c listed subsets, merge them into the running best, read its objective back
template <class Count, class Round>
int window_loop(double U, double LBmax, const char *what, Count count_in, Round round_them)
{
    int rc;
    double lo = -1.0, best = INFINITY;
    int idle = 0;                                   // counting scans since a window last rounded a subset
    while (true) {
        const double hi = std::min(std::min(U, best), LBmax);
        if (!(lo < hi)) break;
        double T = hi;
        unsigned long long c = 0;
        idle++;
        if ((rc = count_in(false, lo, T, &c))) return rc;
        for (int it = 0; c > (unsigned long long)CAND_CAP; it++) {
            if (it >= 200) return fail(BLUEST_ERR_STATE, "more than %lld %ss share one lower bound", (long long)CAND_CAP, what);
            T = lo + 0.5 * (T - lo);
            if (!(T > lo)) break;
            idle++;
            if ((rc = count_in(false, lo, T, &c))) return rc;
        }
        if (!(T > lo) || c > (unsigned long long)CAND_CAP)     // the window cannot advance: never loop on it
            return fail(BLUEST_ERR_STATE, "more than %lld %ss share one lower bound", (long long)CAND_CAP, what);
        if (idle >= MAX_IDLE_SCANS)                             // checked once per window, halvings included
            return fail(BLUEST_ERR_STATE, "%d counting scans without a %s to round: the lower bounds cluster too "
                        "closely for windows of %lld (more than that many share one lower bound)", idle, what, (long long)CAND_CAP);
        if (c > 0) {
            if ((rc = count_in(true, lo, T, &c))) return rc;
            c = std::min(c, (unsigned long long)CAND_CAP);
            if ((rc = round_them(c, &best))) return rc;
            idle = 0;
        }
        lo = T;
    }
    return BLUEST_OK;
}

}  // namespace subset_search

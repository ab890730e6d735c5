// staging.hpp -- what the sample-sum entry points (pilot.hip, gsums.hip, fields.hip) share: telling a host pointer from a device
// pointer, and the pair -> thread map of the pilot statistics.
#pragma once
#include "common.hpp"

namespace {

bool on_device(const void *p)
{
    hipPointerAttribute_t a;
    const hipError_t e = hipPointerGetAttributes(&a, p);
    if (e != hipSuccess) { (void)hipGetLastError(); return false; }
    return a.type == hipMemoryTypeDevice || a.type == hipMemoryTypeManaged;
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

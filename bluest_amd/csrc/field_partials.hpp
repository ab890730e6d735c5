// field_partials.hpp -- the per-chunk work of bluest_field_sums (fields.hip) and bluest_field_weighted_moments (field_moments.hip)
// for a caller in another unit: the chunk records the kernels read and one launch of them over a table that lies on the device.
// field_accum.hip (Part 19) drives them with tables of its own; the one-shot entry points go through the same launches, so a
// chunk has one value whoever asks for it.
#pragma once
#include "common.hpp"

namespace bluest_partials {

struct FChunk {
    const double *src;      // row 0 of the chunk (device address)
    int64_t part;           // where the chunk's W partial sums start, in doubles
    int64_t W;              // column-components per row: sizes[s] * d
    int32_t rows;
};

struct ZChunk {
    const double *src;      // row 0 of the chunk (device address)
    const double *shift;    // the segment's first sample (device address): L d values
    int64_t part;           // where the chunk's 2 d partial sums start, in doubles
    int32_t rows, L;
    int32_t col0;           // the segment's first coefficient
    int32_t sb;             // field_moments_rows
};

// k_fsum_partial over table[0 .. n): part[chunk.part + col] = the chunk's sum of column-component col; Wmax: the widest W of them
hipError_t launch_fsum_partial(const FChunk *table, size_t n, int64_t Wmax, double *part, hipStream_t st);

// The shape of the moment kernels follows (L, d) only.  field_moments_rows: rows per sub-block of k_fmom_staged, 0 for
// k_fmom_wide; field_moments_split: k_fmom_wide with a workgroup per class, the chunk's eight class sums [class][2 d] left to
// the fold; field_moments_lds: doubles of LDS a workgroup of that shape takes.
int field_moments_rows(int L, int64_t d);
bool field_moments_split(int L, int64_t d);
int field_moments_lds(int L, int64_t d);

// k_fmom_staged / k_fmom_wide<split> over table[0 .. n), chunks of ONE kernel shape (`split`; wide follows d); lds_doubles: the
// largest field_moments_lds of their segments
hipError_t launch_fmom_partial(const ZChunk *table, size_t n, bool split, int lds_doubles, int64_t d, const double *coef, double *part,
                               hipStream_t st);

}  // namespace bluest_partials

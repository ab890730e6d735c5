// field_op_layout.hpp -- the host side of a field operator (Part 18 of include/bluest_hip.h; field_map.hip): the checks of a CSR
// matrix and the layout the two kernels of bluest_field_map read.  Plain C++: nothing here touches the device, so both can be
// built and run without one (tests/test_field_maps_host.py compiles a small program over this header).
//
// The layout.  The rows are cut into slices of FM_SLICE = 64 consecutive rows, one wavefront's worth: lane = row.
//   short rows (at most `strip` entries; every finite-element prolongation) live in a sliced ELL: slice t owns the slots
//       [slice_at[t], slice_at[t + 1]), its width W_t = the longest short row of the slice, entry k of lane's row at slot
//       slice_at[t] + k * 64 + lane -- so the 64 lanes read 64 consecutive indices and 64 consecutive coefficients per k.  The
//       entries keep their STORED order.  A padded slot holds index 0 and coefficient 0.0 and is never executed: the kernel runs
//       on len[row], kept apart.
//   long rows (more than `strip` entries: dense functionals) keep their CSR form, the rows one after the other in long_idx /
//       long_val, row j of them at [long_at[j], long_at[j + 1]), long_row[j] its row number.  In the ELL such a row has len = -1:
//       the short kernel neither walks nor writes it.  The rows past q that fill the last slice have len = -1 too.  Consecutive
//       long rows with the same column sequence are listed as a bundle (bundle_at), at most FM_BUNDLE = 8 of them.
// Which of the two a row gets follows from its length only.
#pragma once
#include <algorithm>
#include <cmath>
#include <cstddef>
#include <cstdint>
#include <cstdio>
#include <string>
#include <vector>

namespace {

constexpr int FM_SLICE = 64;

// why (q, d, indptr, indices, data) is not an operator of Part 18, or "" if it is one
inline std::string check_field_csr(int64_t q, int64_t d, const int64_t *indptr, const int32_t *indices, const double *data)
{
    char msg[160];
    if (q < 1 || d < 1) {
        snprintf(msg, sizeof msg, "q=%lld, d=%lld: an operator has at least one row and one column", (long long)q, (long long)d);
        return msg;
    }
    if (q > 0x7fffffffLL || d > 0x7fffffffLL) {
        snprintf(msg, sizeof msg, "q=%lld, d=%lld: more than 2^31 - 1 rows or columns", (long long)q, (long long)d);
        return msg;
    }
    if (!indptr) return "indptr is null";
    if (indptr[0] != 0) {
        snprintf(msg, sizeof msg, "indptr[0]=%lld: it must be 0", (long long)indptr[0]);
        return msg;
    }
    for (int64_t r = 0; r < q; r++)
        if (indptr[r + 1] < indptr[r]) {
            snprintf(msg, sizeof msg, "indptr decreases at row %lld", (long long)r);
            return msg;
        }
    const int64_t nnz = indptr[q];
    if (nnz > 0x7fffffffLL) {
        snprintf(msg, sizeof msg, "nnz=%lld: more than 2^31 - 1 entries", (long long)nnz);
        return msg;
    }
    if (nnz > 0 && (!indices || !data)) return "indices or data is null";
    for (int64_t k = 0; k < nnz; k++) {
        if (indices[k] < 0 || indices[k] >= d) {
            snprintf(msg, sizeof msg, "indices[%lld]=%d outside 0..%lld", (long long)k, indices[k], (long long)d - 1);
            return msg;
        }
        if (!std::isfinite(data[k])) {
            snprintf(msg, sizeof msg, "data[%lld]=%g: the coefficients must be finite", (long long)k, data[k]);
            return msg;
        }
    }
    return "";
}

struct FieldOpLayout {
    int64_t q = 0, d = 0, nnz = 0, nslices = 0;
    std::vector<int32_t> len;           // nslices * 64: the length of a short row; -1 for a long row and past q
    std::vector<int64_t> slice_at;      // nslices + 1
    std::vector<int32_t> ell_idx;       // slice_at[nslices] slots
    std::vector<double> ell_val;
    std::vector<int32_t> long_row;      // the rows with more than `strip` entries, ascending
    std::vector<int64_t> long_at;       // their number + 1
    std::vector<int32_t> long_idx;
    std::vector<double> long_val;
    std::vector<int32_t> bundle_at;     // bundles + 1: bundle b = the long rows [bundle_at[b], bundle_at[b + 1]), numbered as in long_row
};

constexpr int FM_BUNDLE = 8;            // the most long rows a bundle holds

// a CSR that check_field_csr passed
inline FieldOpLayout layout_field_csr(int64_t q, int64_t d, const int64_t *indptr, const int32_t *indices, const double *data, int64_t strip)
{
    FieldOpLayout lay;
    lay.q = q; lay.d = d; lay.nnz = indptr[q];
    lay.nslices = (q - 1) / FM_SLICE + 1;
    lay.len.assign((size_t)lay.nslices * FM_SLICE, -1);
    lay.slice_at.assign((size_t)lay.nslices + 1, 0);
    lay.long_at.push_back(0);
    for (int64_t t = 0; t < lay.nslices; t++) {
        const int64_t r0 = t * FM_SLICE, r1 = std::min(q, r0 + FM_SLICE);
        int64_t width = 0;
        for (int64_t r = r0; r < r1; r++) {
            const int64_t n = indptr[r + 1] - indptr[r];
            if (n <= strip) {
                lay.len[(size_t)r] = (int32_t)n;
                width = std::max(width, n);
            } else {
                lay.long_row.push_back((int32_t)r);
                lay.long_idx.insert(lay.long_idx.end(), indices + indptr[r], indices + indptr[r + 1]);
                lay.long_val.insert(lay.long_val.end(), data + indptr[r], data + indptr[r + 1]);
                lay.long_at.push_back((int64_t)lay.long_idx.size());
            }
        }
        const size_t at = lay.ell_idx.size();
        lay.ell_idx.resize(at + (size_t)width * FM_SLICE, 0);
        lay.ell_val.resize(at + (size_t)width * FM_SLICE, 0.0);
        for (int64_t r = r0; r < r1; r++) {
            const int32_t n = lay.len[(size_t)r];
            for (int32_t k = 0; k < n; k++) {
                lay.ell_idx[at + (size_t)k * FM_SLICE + (size_t)(r - r0)] = indices[indptr[r] + k];
                lay.ell_val[at + (size_t)k * FM_SLICE + (size_t)(r - r0)] = data[indptr[r] + k];
            }
        }
        lay.slice_at[(size_t)t + 1] = (int64_t)lay.ell_idx.size();
    }
    // consecutive long rows that name the same columns in the same order (the rows of a dense functional, of a reduced basis) form
    // a bundle of at most FM_BUNDLE rows: the kernel gathers the values once for all of them.  It changes no bit: every row keeps
    // its own chains.
    lay.bundle_at.push_back(0);
    for (size_t j = 1; j <= lay.long_row.size(); j++) {
        const size_t first = (size_t)lay.bundle_at.back();
        const int64_t n = lay.long_at[first + 1] - lay.long_at[first];
        const bool same = j < lay.long_row.size() && j - first < (size_t)FM_BUNDLE && lay.long_at[j + 1] - lay.long_at[j] == n &&
                          std::equal(lay.long_idx.begin() + lay.long_at[first], lay.long_idx.begin() + lay.long_at[first + 1],
                                     lay.long_idx.begin() + lay.long_at[j]);
        if (!same) lay.bundle_at.push_back((int32_t)j);
    }
    return lay;
}

// row r of the laid-out operator applied to y [d], by the rule of Part 18: what the kernels compute, on the host (for tests)
inline double apply_field_row(const FieldOpLayout &lay, int64_t r, const double *y, int64_t strip)
{
    const int32_t n = lay.len[(size_t)r];
    if (n >= 0) {
        const int64_t t = r / FM_SLICE, lane = r % FM_SLICE;
        double p = 0.0;
        for (int32_t k = 0; k < n; k++) {
            const size_t slot = (size_t)lay.slice_at[(size_t)t] + (size_t)k * FM_SLICE + (size_t)lane;
            p = std::fma(lay.ell_val[slot], y[lay.ell_idx[slot]], p);
        }
        return p;
    }
    const size_t j = (size_t)(std::lower_bound(lay.long_row.begin(), lay.long_row.end(), (int32_t)r) - lay.long_row.begin());
    double total = 0.0;
    for (int64_t a = lay.long_at[j]; a < lay.long_at[j + 1]; a += strip) {
        double p = 0.0;
        for (int64_t k = a; k < std::min(a + strip, lay.long_at[j + 1]); k++) p = std::fma(lay.long_val[(size_t)k], y[lay.long_idx[(size_t)k]], p);
        total = total + p;
    }
    return total;
}

}  // namespace

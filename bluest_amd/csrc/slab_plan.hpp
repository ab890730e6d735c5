// slab_plan.hpp -- how the host segments of a ragged sample-sum call (staging.hpp) are cut into slabs of one staging buffer.
// Plain C++: nothing here touches the device, so the plan can be built and tested without one (tests/test_slab_plan_host.py).
//
// The contract the entry points rely on: a slab boundary never shows in a result.  It holds because every piece but the last of
// its segment is a whole number of chunks, so the chunks of a segment are the same whatever the budget is.
#pragma once
#include <algorithm>
#include <cstddef>
#include <cstdint>
#include <vector>

namespace {

struct Piece {              // rows [first, first + rows) of a host segment, staged at `at` bytes of its slab
    int64_t seg, first, rows;
    size_t at;
    int slab;
};

struct SlabPlan {
    std::vector<Piece> pieces;          // segment by segment, rows ascending; the slab numbers ascend without gaps
    std::vector<size_t> slab_used;      // bytes per slab
    size_t stage_bytes = 0;             // the largest of them: what the staging buffer must hold
    size_t budget = 0;                  // the budget in effect
};

// row_bytes[s]: the bytes of one row of segment s (all of its planes); staged[s]: segment s lies in host memory and has rows.
// Whole chunks only, each piece 256-byte aligned.  The budget in effect is at least the widest chunk of the call (staged or
// not) + 256, so an empty slab always fits a chunk and no slab stays empty.
inline SlabPlan plan_slabs(int64_t S, const int64_t *counts, const size_t *row_bytes, const char *staged, int64_t chunk, size_t budget)
{
    SlabPlan plan;
    size_t widest = 0;
    for (int64_t s = 0; s < S; s++) widest = std::max(widest, row_bytes[s]);
    plan.budget = budget = std::max(budget, (size_t)chunk * widest + 256);
    size_t used = 0;
    int slab = 0;
    bool open = false;
    for (int64_t s = 0; s < S; s++) {
        if (!staged[s]) continue;
        int64_t a = 0;
        while (a < counts[s]) {
            const int64_t rest = counts[s] - a;
            int64_t fit = (int64_t)((budget - used) / row_bytes[s]);
            if (fit < rest) fit -= fit % chunk;
            if (fit <= 0) {                 // (only a slab that holds something is ever too full for a chunk)
                plan.slab_used.push_back(used);
                slab++;
                used = 0;
                continue;
            }
            const int64_t rows = std::min(rest, fit);
            plan.pieces.push_back(Piece{s, a, rows, used, slab});
            used = std::min(budget, (used + (size_t)rows * row_bytes[s] + 255) & ~(size_t)255);
            open = true;
            a += rows;
        }
    }
    if (open) plan.slab_used.push_back(used);
    if (!plan.slab_used.empty()) plan.stage_bytes = *std::max_element(plan.slab_used.begin(), plan.slab_used.end());
    return plan;
}

}  // namespace

// Prints the slab plans (bluest_amd/csrc/slab_plan.hpp) of the cases on standard input, for tests/test_slab_plan_host.py.
//   in,  per case:  S chunk budget, then S times: count row_bytes staged
//   out, per case:  "plan <budget in effect> <stage_bytes> <slabs> <pieces>", "used <bytes per slab> ...", then per piece
//                   "piece <seg> <first> <rows> <at> <slab>"
#include <cstdio>

#include "slab_plan.hpp"

int main()
{
    long long S, chunk;
    unsigned long long budget;
    while (std::scanf("%lld %lld %llu", &S, &chunk, &budget) == 3) {
        std::vector<int64_t> counts((size_t)S);
        std::vector<size_t> row_bytes((size_t)S);
        std::vector<char> staged((size_t)S);
        for (long long s = 0; s < S; s++) {
            long long n;
            unsigned long long rb;
            int st;
            if (std::scanf("%lld %llu %d", &n, &rb, &st) != 3) return 2;
            counts[s] = n;
            row_bytes[s] = (size_t)rb;
            staged[s] = (char)st;
        }
        const SlabPlan plan = plan_slabs(S, counts.data(), row_bytes.data(), staged.data(), chunk, (size_t)budget);
        std::printf("plan %zu %zu %zu %zu\n", plan.budget, plan.stage_bytes, plan.slab_used.size(), plan.pieces.size());
        std::printf("used");
        for (size_t u : plan.slab_used) std::printf(" %zu", u);
        std::printf("\n");
        for (const Piece &p : plan.pieces)
            std::printf("piece %lld %lld %lld %zu %d\n", (long long)p.seg, (long long)p.first, (long long)p.rows, p.at, p.slab);
    }
    return 0;
}

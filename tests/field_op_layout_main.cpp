// The host side of a field operator (bluest_amd/csrc/field_op_layout.hpp) without a GPU: reads cases from the file named on the
// command line and prints, per case, what the checks say or the laid-out operator applied to the case's samples.
//   case:   q d nnz N strip, then indptr (q + 1), indices (nnz), data (nnz, as %a), y (N x d, as %a)
//   answer: "ERR <message>", or "OK <slices> <long rows> <ELL slots> <bundles of long rows>" and N lines of q values (%a)
// tests/test_field_maps_host.py compiles it with g++ and compares the values, bit for bit, with tests/field_map_ref.py.
#include "../bluest_amd/csrc/field_op_layout.hpp"

int main(int argc, char **argv)
{
    if (argc != 2) return 2;
    FILE *f = fopen(argv[1], "r");
    if (!f) return 2;
    long long q, d, nnz, N, strip;
    while (fscanf(f, "%lld %lld %lld %lld %lld", &q, &d, &nnz, &N, &strip) == 5) {
        std::vector<int64_t> indptr((size_t)std::max(q, 0LL) + 1);
        std::vector<int32_t> indices((size_t)nnz);
        std::vector<double> data((size_t)nnz), y((size_t)(N * std::max(d, 0LL)));
        for (auto &v : indptr) { long long x; if (fscanf(f, "%lld", &x) != 1) return 3; v = x; }
        for (auto &v : indices) { int x; if (fscanf(f, "%d", &x) != 1) return 3; v = x; }
        for (auto &v : data) if (fscanf(f, "%la", &v) != 1) return 3;
        for (auto &v : y) if (fscanf(f, "%la", &v) != 1) return 3;
        const std::string why = check_field_csr(q, d, indptr.data(), indices.data(), data.data());
        if (!why.empty()) {
            printf("ERR %s\n", why.c_str());
            continue;
        }
        const FieldOpLayout lay = layout_field_csr(q, d, indptr.data(), indices.data(), data.data(), strip);
        printf("OK %lld %zu %zu %zu\n", (long long)lay.nslices, lay.long_row.size(), lay.ell_idx.size(), lay.bundle_at.size() - 1);
        for (long long s = 0; s < N; s++) {
            for (long long r = 0; r < q; r++) printf("%a ", apply_field_row(lay, r, y.data() + s * d, strip));
            printf("\n");
        }
    }
    fclose(f);
    return 0;
}

// plan.hpp -- the evaluation plan (Part 2 of include/bluest_hip.h) as the translation units see it.
#pragma once
#include "solve.hpp"

// Tile = 64 groups of equal size k of one output, lane = group.  Per group S(k) = ne + ni (+1 to make it even) 8-byte SLOTS:
// slots [0, ni) hold the k model indices as bytes (ni = ceil(k/8)), slots [ni, ni+ne) the ne = k(k+1)/2 packed-symmetric
// entries of the group's inverse.  Slots are stored in PAIRS, pair-major: pair p of lane l sits at doubles [p*128 + 2l, +2),
// so one wave-instruction loads 16 bytes per lane, 1 KiB contiguous, and the indices come with the same loads (k = 5: 8 loads
// per tile instead of the 15 + 5 of the 8-byte-per-lane form of rounds 1-2; step 14.4 -> 14.1 us at the headline size).
struct TileDesc {
    int64_t val_off;  // doubles: first slot pair of the tile
    int64_t grad_off; // position of the tile's first group inside the concatenated gradient
    int32_t n_valid;  // groups in this tile (<= 64); bit 30 set on the first tile of an output
    int16_t k, out;
};
__host__ __device__ constexpr int tile_ne(int k) { return k * (k + 1) / 2; }
__host__ __device__ constexpr int tile_ni(int k) { return (k + 7) / 8; }
__host__ __device__ constexpr int tile_slots(int k) { return (tile_ne(k) + tile_ni(k) + 1) & ~1; }
__host__ __device__ constexpr int tile_pairs(int k) { return tile_slots(k) / 2; }
// offset (doubles, relative to the tile) of slot sl of lane l
__host__ __device__ constexpr int64_t tile_slot_off(int sl, int lane) { return (int64_t)(sl >> 1) * 128 + lane * 2 + (sl & 1); }

// descriptor t through scalar loads into scalar registers; t must be wave-uniform.  (The descriptors are written at set-up and
// by nobody afterwards; the constant address space is what lets the load be a scalar one behind a kernarg_now, see uniform_word.)
__device__ __forceinline__ TileDesc tile_desc_uniform(const TileDesc *__restrict__ tiles, int64_t t)
{
    static_assert(sizeof(TileDesc) == 24, "three 64-bit words");
    const auto *w = (const __attribute__((address_space(4))) uint64_t *)(tiles + t);
    const uint64_t w0 = w[0], w1 = w[1], w2 = w[2];
    TileDesc td;
    td.val_off = (int64_t)w0; td.grad_off = (int64_t)w1; td.n_valid = (int32_t)(uint32_t)w2;
    td.k = (int16_t)(uint16_t)(w2 >> 32); td.out = (int16_t)(uint16_t)(w2 >> 48);
    return td;
}


struct OutputDesc {
    int K = 0;
    std::vector<int64_t> sizes;    // K entries
    std::vector<int64_t> groups;   // concat (L_k * k), host copy (kept: restricted plans, descriptors)
    std::vector<int64_t> mapping;  // L_o global indices
    int64_t L_o = 0;
    int64_t n_inv = 0;             // doubles of the reference-layout inverses: sum L_k k^2
    double *d_invcov = nullptr;    // DEVICE, reference layout concat (L_k * k * k): pinv output or uploaded; lives as long as the plan
    uint8_t *d_groups = nullptr;   // DEVICE copy of `groups`, one byte per model index (n <= 64): 8x less to push over PCIe
                                   // than the int64 list (11 MB at K_tot = 245 505); shared with output 0 when the lists are identical
    bool owns_groups = false;
    std::vector<double> h_C;       // the covariance (N x N) when the output was given by it (host copy: 5 KB; the matrix-free evaluation uploads it)
};

struct bluest_plan_s {
    int device = -1;      // HIP device the plan's memory lives on (current device at bluest_plan_create)
    int N = 0;
    int64_t L = 0;
    std::vector<OutputDesc> outs;
    bool finalized = false;
    int max_cand = 0;
    int iters = 1;  // chunk = 256*iters entries
    bool shared = false;  // all outputs have identical groups + mapping
    bool identity = false; // ... and that mapping is the identity (local index = global index for every output)
    int kmax = 0;         // largest group size over the outputs (picks the KU instantiation of the tile kernels)
    bool spg_small = false;   // small plan: the gradient tiles of the accepted SPG point run inside the single-workgroup finishing
                              // kernel (bluest_spg_finish, bluest_spg_window); else every evaluation is the fused solve + gradient launch
    int fused_bpo = 0;    // workgroups of k_solve_grad per output when that is the same for every output, else 0
    int fused_tpb = 15;   // tiles per workgroup of k_solve_grad for this plan (tile list is padded to it per output)
    bool tile_nt = true;  // k_solve_grad streams its tiles with non-temporal loads (same-box A/B over six shapes: 12.8 vs 14.3 us
                          // per step at the headline size, the others within +-2 %; BLUEST_TILE_NT=0 switches it off)
    const int32_t *gate = nullptr;  // optional device word: 0 = skip the plan's kernels (bluest_plan_set_gate)
    bool always_v = false;          // compute v in every solve (device-side SPG keeps the accepted trial's v)
    int nsym = 0;
    int64_t n_chunks = 0, n_tiles = 0, grad_len = 0;
    std::vector<int64_t> grad_off;
    int64_t phi_bytes = 0, grad_bytes = 0;
    // device
    double *d_vals = nullptr;
    int32_t *d_cols = nullptr;          // columns of the Phi layout; holds uint16 entries when cols16 (allocation vectors of <= 65 536 entries)
    bool cols16 = false;
    int phi_ob_forced = 0;              // BLUEST_PHI_OB=2|4|8 at finalize (A/B switch): OB of the shared Phi pass, 0: phi_ob()'s rule
    RowDesc *d_rows = nullptr;
    TileDesc *d_tiles = nullptr;
    double *d_tvals = nullptr;   // tiles: slot pairs (see TileDesc)
    int32_t *d_invmap = nullptr;
    int64_t *d_goff = nullptr;
    FoldReg fold_reg = {0, 0, nullptr};          // regular rows: fixed partial strides per destination class (solve.hpp), else {0, 0}
    int32_t *d_pslot = nullptr;         // chunk -> partial slot (regular rows; per structure)
    int64_t partial_stride = 0;         // partial slots per candidate
    int slots_per_output = 0;
    double2 *d_partial = nullptr;
    double *d_v = nullptr;       // workspace for eval
    void *d_arena = nullptr;     // ONE device allocation behind all the d_* arrays (hipMalloc is 1-3 ms a piece on a busy process)
    void *d_scratch = nullptr;   // set-up scratch of bluest_plan_add_output_cov (C, groups, inverses), reused across outputs
    size_t scratch_bytes = 0;
    int32_t *d_status = nullptr; // workspace for eval when caller passes NULL
    unsigned int *d_ticket = nullptr;   // [0] arrival counter of the fused solve + line-search decision (bluest_plan_eval_decide);
                                        // [16] arrival counter of the workgroups of a predicated-off launch that still decides
    // second-order finish (newton.hip): descriptor blob of the master problem (plain hipMalloc, grown on demand) and the
    // host-side global -> local group maps it is built from
    // matrix-free evaluation (matfree.hip): chosen at finalize for plans that qualify
    bool matfree = false;        // Phi pass and gradient pass matrix-free
    bool mf_gradient = false;    // gradient pass matrix-free (also true when matfree): the stored Phi pass + k_solve_grad_mf folding its partials
    void *mf = nullptr;          // MfState (matfree.hip)
    void *d_master = nullptr;
    size_t master_bytes = 0;
    std::vector<std::vector<int32_t>> inv_host;
};

// current device for the lifetime of the object (a plan's memory and kernels live on plan->device)
struct DeviceScope {
    int prev = -1;
    bool switched = false;
    explicit DeviceScope(int dev)
    {
        if (hipGetDevice(&prev) == hipSuccess && prev != dev && dev >= 0) switched = hipSetDevice(dev) == hipSuccess;
    }
    ~DeviceScope() { if (switched) (void)hipSetDevice(prev); }
};


// ---- tile device code shared by plan.hip (gradient pass, fused kernel) and spg.hip (small-plan finish kernel) ----
// the slot pairs of one lane's group, PU pairs of registers (PU >= tile_pairs(K)); loaded with 16-byte loads
typedef double tile_d2v __attribute__((ext_vector_type(2)));
template <int PU, bool NT = false>
__device__ __forceinline__ void tile_load(double2 (&pr)[PU], const double *__restrict__ tile, int lane, int n_pairs)
{   // tile = tvals + td.val_off; NT: non-temporal loads (the fused kernel's stream, see bluest_plan_s::tile_nt).  The lane's
    // offset is ONE 32-bit byte offset for the first four pairs (an instruction's own offset ends below 4096; behind them the
    // compiler folds the 4096 into a 64-bit lane address), so a wave-uniform tile keeps its base in scalar registers
    const char *base = reinterpret_cast<const char *>(tile);
    const uint32_t lo = 16u * (uint32_t)lane;
#pragma unroll
    for (int i = 0; i < PU; i++)
        if (i < n_pairs) {
            const char *p = (base + (lo + 4096u * (i >> 2))) + 1024 * (i & 3);
            if (NT) { const tile_d2v v = __builtin_nontemporal_load(reinterpret_cast<const tile_d2v *>(p)); pr[i] = make_double2(v.x, v.y); }
            else pr[i] = *reinterpret_cast<const double2 *>(p);
        }
}
template <int PU>
__device__ __forceinline__ double tile_slot(const double2 (&pr)[PU], int sl) { return (sl & 1) ? pr[sl >> 1].y : pr[sl >> 1].x; }   // sl static after unrolling

// the quadratic form of one group from its slot pairs: q = v_g^T S v_g (packed symmetric S, K static);
// q = sum_j v_j (s_jj v_j + 2 sum_{l>j} s_jl v_l)
template <int K, int PU>
__device__ __forceinline__ double tile_form(const double2 (&pr)[PU], const double *__restrict__ vc)
{
    constexpr int NI = tile_ni(K);
    double vj[K];
#pragma unroll
    for (int j = 0; j < K; j++) {      // model j of the group: byte j & 7 of index slot j >> 3, taken from the dword that holds it
        const double sl = tile_slot(pr, j >> 3);
        const unsigned w = (unsigned)((j & 4) ? __double2hiint(sl) : __double2loint(sl));
        vj[j] = vc[(w >> (8 * (j & 3))) & 0xffu];
    }
    double q = 0.0;
    int e = NI;
#pragma unroll
    for (int j = 0; j < K; j++) {
        double t = 0.0;
#pragma unroll
        for (int l = j + 1; l < K; l++) t = fma(tile_slot(pr, e + (l - j)), vj[l], t);
        t = fma(tile_slot(pr, e), vj[j], 2.0 * t);
        q = fma(vj[j], t, q);
        e += K - j;
    }
    return q;
}

// gradient pass: one wavefront per tile, lane = group
template <int K>
__device__ __forceinline__ void grad_tile(const TileDesc &td, const double *__restrict__ tvals, const double *__restrict__ v,
                                          const int32_t *__restrict__ status, int N, int n_out, int n_cand,
                                          double *__restrict__ grad, int64_t grad_stride, int lane)
{
    double2 pr[tile_pairs(K)];
    tile_load(pr, tvals + td.val_off, lane, tile_pairs(K));
    for (int c = 0; c < n_cand; c++) {
        const int64_t eo = (int64_t)c * n_out + td.out;
        const double q = tile_form<K>(pr, v + eo * N);
        if (lane < (td.n_valid & 0xffff))
            grad[(int64_t)c * grad_stride + td.grad_off + lane] = (status[eo] == BLUEST_EVAL_INF) ? INFINITY : -q;
    }
}

// generic k (13..BLUEST_MAX_GROUP): slots re-read per candidate, no big register arrays
__device__ __forceinline__ void grad_tile_generic(const TileDesc &td, const double *__restrict__ tvals, const double *__restrict__ v,
                                                  const int32_t *__restrict__ status, int N, int n_out, int n_cand,
                                                  double *__restrict__ grad, int64_t grad_stride, int lane)
{
    const int K = td.k;
    const double *tile = tvals + td.val_off;
    const int ni = tile_ni(K);
    auto model = [&](int j) { return (int)reinterpret_cast<const uint8_t *>(tile + tile_slot_off(j >> 3, lane))[j & 7]; };
    for (int c = 0; c < n_cand; c++) {
        const int64_t eo = (int64_t)c * n_out + td.out;
        const double *vc = v + eo * N;
        double q = 0.0;
        int e = ni;
        for (int j = 0; j < K; j++) {
            const double vjj = vc[model(j)];
            double t = 0.0;
            for (int l = j + 1; l < K; l++) t = fma(tile[tile_slot_off(e + (l - j), lane)], vc[model(l)], t);
            t = fma(tile[tile_slot_off(e, lane)], vjj, 2.0 * t);
            q = fma(vjj, t, q);
            e += K - j;
        }
        if (lane < (td.n_valid & 0xffff))
            grad[(int64_t)c * grad_stride + td.grad_off + lane] = (status[eo] == BLUEST_EVAL_INF) ? INFINITY : -q;
    }
}


// single-output plans: the multiplicative update of phase 1 (newton.hip, k_ma_update) done by the fused solve + gradient kernel's
// tile wavefronts instead of writing the gradient: x_i <- x_i cc_i (q_i / s_0) / (V / s_0), m_i = cc_i x_i (x == NULL: off)
struct MaTail { double *x; const double *cc; double *m; const double *s; };

int plan_ready(bluest_plan_t plan, int n_cand);
// the library's device block cache (plan.hip)
hipError_t pool_alloc(void **p, size_t bytes);
hipError_t pool_free(void *p, bool recycle = true);
// matrix-free evaluation (matfree.hip)
int mf_finalize(bluest_plan_t plan);
void mf_release(bluest_plan_s *p);
int mf_phi_record(bluest_plan_t plan, const double *m_dev, double *rec_dev, const double **rec_used, hipStream_t st);
int mf_solve_grad(bluest_plan_t plan, const double *rec_dev, double delta, double *var_dev, int32_t *status_dev, double *grad_dev, hipStream_t st,
                  MaTail ma = MaTail{nullptr, nullptr, nullptr, nullptr});
int mf_grad(bluest_plan_t plan, const double *v_dev, const int32_t *status_dev, double *grad_dev, hipStream_t st);
void mf_instantiation(bluest_plan_t plan, int32_t *nw, int32_t *nt, int32_t *ku);
void mf_instantiation_set(int axis, std::vector<int32_t> &s);

// plan.hip -- Part 2 of include/bluest_hip.h: the evaluation plan of one (multi-output) sample-allocation problem on MI355X
// (gfx950 / CDNA4).
//
// What is computed (reference files bluest/*.py, bluest/cmisc.cpp; cited per function in include/bluest_hip.h):
//   Phi_o(m) = sum_i m_i R_i^T C_i^-1 R_i      (misc.py:459-461, cmisc.cpp:25-40)
//   V_o      = (Phi_o[idx,idx]^-1)_00          (misc.py:463-477, :490)
//   grad_o,i = -v[g_i]^T C_i^-1 v[g_i]         (misc.py:493, cmisc.cpp:58-72), v = row 0 of pinv(Phi_o)
// for every output o of a multi-output problem and a batch of candidate allocations m, all float64.
//
// Design: HBM/L2-streaming integer + f64 work with ~0.2 flop/byte, so there is no MFMA; the levers are
// coalescing, bytes per entry, dependent round trips and launch count.
//   * Phi pass : destination-major symmetric CSR of psi, cut into wave-sized chunks; one wavefront streams one chunk with
//                16-byte loads and gathers m from L2; fixed-order butterfly sum => bit-reproducible (no float atomics).
//   * solve    : per (candidate, output): quads of lanes fold the chunk partials per row -> Phi in LDS; one wavefront holds
//                the restricted, permuted matrix in registers and eliminates by Gauss-Jordan (solve.hpp).
//   * grad pass: group-major tiles of 64 groups, lane = group; per group the model indices and the packed-symmetric inverse as
//                8-byte slots stored in pairs, so every wave-instruction reads 16 bytes per lane, 1 KiB contiguous (TileDesc,
//                plan.hpp); fused with the solve for the single-candidate evaluation (k_solve_grad: one solver wavefront, the
//                tile wavefronts streaming -- non-temporal loads -- while it factorises; tiles per workgroup chosen per plan
//                so that the workgroups cover every compute unit).
//   * What bounds a step after round 3: the two copies of the inverses (Phi layout + tiles) evict each other from the L2s; see
//                DESIGN.md section 4 and profiles/r03_phi_tiles_negative_result.txt (a single-copy pass measured slower).
// No CPU fallback exists in this library.

#include "common.hpp"

static int g_debug_timing = getenv("BLUEST_DEBUG_TIMING") ? 1 : 0;   // stderr phase times of the set-up entry points
struct PhaseTimer {
    std::chrono::steady_clock::time_point t0 = std::chrono::steady_clock::now();
    const char *what;
    explicit PhaseTimer(const char *w) : what(w) {}
    void lap(const char *phase)
    {
        if (!g_debug_timing) return;
        const auto t1 = std::chrono::steady_clock::now();
        fprintf(stderr, "[bluest timing] %s: %s %.3f ms\n", what, phase, std::chrono::duration<double, std::milli>(t1 - t0).count());
        t0 = t1;
    }
};


#include "plan.hpp"
#include "spg_state.hpp"

// ------------------------------------------------------------------------------------------------------
// Part 2 -- plan kernels
// ------------------------------------------------------------------------------------------------------
// columns (global group indices) are stored as uint16 when the allocation vector has at most 65 536 entries (half the bytes of the
// column stream, which the shared kernel re-reads per pair of outputs), else as int32
template <typename COLT> __device__ __forceinline__ int4 load_cols4(const COLT *p);
template <> __device__ __forceinline__ int4 load_cols4<int32_t>(const int32_t *p) { return *reinterpret_cast<const int4 *>(p); }
template <> __device__ __forceinline__ int4 load_cols4<uint16_t>(const uint16_t *p)
{
    const uint2 w = *reinterpret_cast<const uint2 *>(p);
    return make_int4((int)(w.x & 0xffffu), (int)(w.x >> 16), (int)(w.y & 0xffffu), (int)(w.y >> 16));
}
// Phi pass: one wavefront per chunk of CH = 256*iters entries; lane l owns entries [4l, 4l+4) of each 256-block.
// Prologue of both chunk kernels: what the stream needs arrives in scalar registers with the wavefront (see "Arguments" below), the
// gate of a launch that has one costs two scalar round trips (pointer, word), and the slot of the chunk's partial -- needed behind
// the loop only -- is a scalar load issued behind the stream's first loads by a plan that has a slot table (another keeps the
// chunk number), so no wait stands between the launch and the first streaming load.
// Tail: every workgroup is whole wavefronts and the early exits are wave-uniform, so all 64 lanes reach the reductions, which
// run on the VALU (wave_sum_dpp / wave_max_dpp, common.hpp).
// What the compiler makes of this prologue and of the addressing below is recorded in profiles/r10_isa_counts.txt (tools/isa_counts.py):
// re-check it there after a toolchain update.
// Addressing of both chunk kernels: a wavefront's chunk, its output block and every base of vals / cols / m / partial are
// wave-uniform and live on the SALU; a lane adds one 32-bit byte offset per stream (the loads and the store take the scalar base
// plus that offset).  What makes 32 bits enough: bluest_plan_finalize refuses plans of more than 0x7fffffff0 entries, so a chunk
// number and a position in d_partial (one double2 per chunk and candidate) stay below 2^28, and a chunk is at most 1024 * 256
// entries (2 MiB of values).  Bases are formed in 64 bits.
// With one wavefront per workgroup (the only launch there is) the chunk is blockIdx.x; the wave number of a wider workgroup
// has to be read out of the first lane to be scalar for the compiler too.
template <int WPB> __device__ __forceinline__ uint32_t phi_wave_chunk()
{
    if constexpr (WPB == 1) return blockIdx.x;
    else return blockIdx.x * WPB + (uint32_t)__builtin_amdgcn_readfirstlane((int)(threadIdx.x >> 6));
}
// Arguments of both chunk kernels.  The first 14 dwords of a kernel's argument list arrive in scalar registers with the wavefront
// (kernarg preload, the -mllvm option bluest_amd/build.py gives this unit), so everything the common path needs in front of its first
// streaming load stands there in the form the loads take it, computed once at the launch site: vals, cols, m, pslot, CH = 256 * iters
// (entries of a chunk), the chunk count, one output's values in bytes (per_out_bytes = chunks per output * CH * 8, the step from
// one output's base to the next), n_out with the flags in its top bits (PHI_HAS_GATE: the gate pointer is loaded, one scalar round
// trip, only by a launch that has one) and n_cand.  The others are first needed by the store: they are waited for behind the issue
// of the stream's first loads (phi_late_args), so the round trip to the argument segment runs under the one to the stream.
// Entry: both kernels open with one sweep over a 256-block written out on its own (sweep(std::true_type)).  From the preload entry to
// the issue of the column load and the first output's two value loads a wavefront forms its chunk, one 64-bit base per stream and the
// lane's two 32-bit offsets, nothing else.  The bases of the second and later outputs follow behind an ordering point
// (phi_issue_point), and everything only the stores need -- the slot word, the owner and index of wave_sum_multi, the stride between
// outputs' partials, the loop count -- behind the loads of the first (at most four) outputs and another such point: it runs under a
// round trip that has to be waited for anyway.  All of it is loop-invariant: the loops over the chunk's further 256-blocks and over
// the candidates stand behind the opening sweep and reuse it.  profiles/r10_isa_counts.txt has the listing.
constexpr uint32_t PHI_HAS_GATE = 1u << 31, PHI_N_OUT_MASK = ~PHI_HAS_GATE;
template <class... A> __device__ __forceinline__ void phi_late_args(const A &...a) { kernarg_now(a...); }
// nothing moves across this point, neither in the compiler's passes nor in its instruction scheduler
__device__ __forceinline__ void phi_issue_point()
{
    asm volatile("" ::: "memory");
    __builtin_amdgcn_sched_barrier(0);
}
// the partials are stored through a pointer the compiler knows to be global memory: behind uniform_value_here it has lost that, and
// with a flat store in the loop every vector wait in it was a wait for ALL loads (the columns' wait took the value stream with it)
typedef double PhiPair __attribute__((ext_vector_type(2)));      // (a plain vector type: double2 is a class for the host compiler)
__device__ __forceinline__ void store_partial(char *p, double s, double amax)
{
    PhiPair w;
    w.x = s; w.y = amax;
    *(__attribute__((address_space(1))) PhiPair *)p = w;
}
// the value stream's bases likewise: they are formed in steps, output by output, and are global memory by their type
using PhiStream = const __attribute__((address_space(1))) char *;
__device__ __forceinline__ double2 stream_pair(PhiStream p)
{
    const PhiPair w = *reinterpret_cast<const __attribute__((address_space(1))) PhiPair *>(p);
    return make_double2(w.x, w.y);
}
template <int WPB, typename COLT>
__global__ __launch_bounds__(64 * WPB) void k_phi_chunks(const double *__restrict__ vals, const COLT *__restrict__ cols,
                                                    const double *__restrict__ m, const int32_t *__restrict__ pslot,
                                                    uint32_t CH, uint32_t n_chunks, uint64_t per_out_bytes, uint32_t n_out_flags, int n_cand,
                                                    const int32_t *__restrict__ gate, int64_t m_stride, int64_t pstride,
                                                    int slots_per_output, double2 *__restrict__ partial)
{
    (void)per_out_bytes; (void)slots_per_output;      // (one argument list for both chunk kernels)
    const uint32_t chunk = phi_wave_chunk<WPB>();
    const uint32_t lane = threadIdx.x & 63;
    if (__builtin_expect((n_out_flags & PHI_HAS_GATE) != 0, 0)) { if (uniform_word(gate) == 0) return; }      // device-side predication (SPG line-search slots)
    if (chunk >= n_chunks) return;
    const uint64_t base = (uint64_t)chunk * CH;      // entries in front of this chunk
    const PhiStream vb = (PhiStream)(vals + base);
    const char *cb = reinterpret_cast<const char *>(cols + base);
    const double *mc = m;
    double s = 0.0, amax = 0.0;
    uint32_t vo = lane * 32u, co = lane * (uint32_t)(4 * sizeof(COLT));
    uint32_t iters = 1;
    int32_t slot_ld = 0;
    // one 256-block of the chunk; first: the sweep that opens the kernel, with what only the store needs behind its loads
    auto sweep = [&](auto first) {
        const int4 cc = load_cols4<COLT>(reinterpret_cast<const COLT *>(cb + co));
        const double2 v01 = stream_pair(vb + vo), v23 = stream_pair(vb + vo + 16);
        if constexpr (decltype(first)::value) {
            phi_issue_point();
            iters = uniform_value_here(CH) >> 8;
            phi_late_args(m_stride, pstride, partial);      // (one scalar wait, behind the issue of the stream's loads)
            // where the fold expects this chunk's partial: a scalar load behind that wait, in flight until the store (a plan
            // without a slot table keeps the chunk number)
            if (pslot) slot_ld = uniform_word(pslot + uniform_value_here(chunk));
        }
        const double m0 = mc[cc.x], m1 = mc[cc.y], m2 = mc[cc.z], m3 = mc[cc.w];
        s = fma(v01.x, m0, s);
        s = fma(v01.y, m1, s);
        s = fma(v23.x, m2, s);
        s = fma(v23.y, m3, s);
        amax = fmax(fmax(amax, fmax(fabs(m0), fabs(m1))), fmax(fabs(m2), fabs(m3)));
        vo += 2048u; co += (uint32_t)(256 * sizeof(COLT));
    };
    sweep(std::true_type());
    int64_t pdone = 0;      // candidates' partials in front of this one, in bytes
    uint32_t it = 1;
    for (int c = 0;;) {
        for (; it < iters; it++) sweep(std::false_type());
        s = wave_sum_dpp(s);
        amax = wave_max_dpp(amax);
        const uint32_t slot = pslot ? (uint32_t)uniform_value_here(slot_ld) : chunk;
        char *pc = reinterpret_cast<char *>(uniform_value_here(partial)) + pdone;
        if (lane == 0) store_partial(pc + slot * 16u, s, amax);
        if (++c >= n_cand) break;
        mc += uniform_value_here(m_stride);      // (not hoisted in front of the loop, where they would be waited for)
        pdone += uniform_value_here(pstride) * (int64_t)sizeof(double2);
        // (the next candidate's offsets taken as they are here: a chunk of one 256-block has the same columns for every candidate,
        //  and their load is not to be moved in front of the loops)
        s = 0.0; amax = 0.0; it = 0;
        vo = lane_value_here(lane * 32u); co = lane_value_here(lane * (uint32_t)(4 * sizeof(COLT)));
    }
}

// Phi pass, shared structure: when every output has the same groups and mapping (the usual multi-output case) the
// column indices and the gathered m are common; one wavefront streams the chunk of OB outputs and reads them once.
// vals / partial keep the output-major chunk numbering of the general layout (chunk id = o*ncpo + c).
// Tail: the OB sums are reduced together (wave_sum_multi, common.hpp: the first two levels transpose them into a quarter as
// many registers), and the lane that ends with an output's total stores it -- one store instruction per result register.  An
// output beyond n_out (the tail block streams the last real output again in its place) stores nothing.
template <int OB, int WPB, typename COLT>
__global__ __launch_bounds__(64 * WPB) void k_phi_chunks_shared(const double *__restrict__ vals, const COLT *__restrict__ cols,
                                                           const double *__restrict__ m, const int32_t *__restrict__ pslot,
                                                           uint32_t CH, uint32_t ncpo, uint64_t per_out_bytes, uint32_t n_out_flags, int n_cand,
                                                           const int32_t *__restrict__ gate, int64_t m_stride, int64_t pstride,
                                                           int slots_per_output, double2 *__restrict__ partial)
{
    const uint32_t chunk = phi_wave_chunk<WPB>();
    const uint32_t lane = threadIdx.x & 63;
    if (__builtin_expect((n_out_flags & PHI_HAS_GATE) != 0, 0)) { if (uniform_word(gate) == 0) return; }      // device-side predication (SPG line-search slots)
    if (chunk >= ncpo) return;
    const char *cb = reinterpret_cast<const char *>(cols + (uint64_t)chunk * CH);
    constexpr int NR = wave_sum_multi_regs(OB);
    // bases of the outputs o0 + oo; the first one here, the others behind the issue of its loads
    PhiStream vb[OB];
    vb[0] = (PhiStream)(vals + (uint64_t)(blockIdx.y * OB * ncpo + chunk) * CH);
    // this lane's results after wave_sum_multi: the position of its partial but for the slot, in double2, and whether it stores one
    uint32_t opos[NR];
    bool mine[NR];
    const double *mc = m;
    double s[OB];
#pragma unroll
    for (int oo = 0; oo < OB; oo++) s[oo] = 0.0;
    double amax = 0.0;
    uint32_t vo = lane * 32u, co = lane * (uint32_t)(4 * sizeof(COLT));
    uint32_t iters = 1;
    int32_t slot_ld = 0;
    // one 256-block of the chunk; first: the sweep that opens the kernel, with the loop-invariant work behind the issue of its loads
    auto sweep = [&](auto first) {
        constexpr bool FIRST = decltype(first)::value;
        const int4 cc = load_cols4<COLT>(reinterpret_cast<const COLT *>(cb + co));
        double2 v01[OB], v23[OB];
        v01[0] = stream_pair(vb[0] + vo);
        v23[0] = stream_pair(vb[0] + vo + 16);
        if constexpr (FIRST) {
            phi_issue_point();
            // output o0 + oo, clamped to the last one: each base is the one before it plus one output's values, or the same again
            const uint32_t n_out = n_out_flags & PHI_N_OUT_MASK, o0 = blockIdx.y * OB;
#pragma unroll
            for (int oo = 1; oo < OB; oo++) vb[oo] = vb[oo - 1] + (o0 + oo < n_out ? per_out_bytes : 0);
        }
#pragma unroll
        for (int oo = 1; oo < OB; oo++) {
            v01[oo] = stream_pair(vb[oo] + vo);
            v23[oo] = stream_pair(vb[oo] + vo + 16);
            // (behind the loads of at most four outputs: the point orders the loads around it, and OB = 8 with all sixteen
            //  in front of it takes 100 registers instead of 62)
            if constexpr (FIRST) if (oo == (OB < 4 ? OB : 4) - 1) {
                phi_issue_point();
                const uint32_t n_out = n_out_flags & PHI_N_OUT_MASK, o0 = blockIdx.y * OB;
                iters = CH >> 8;
#pragma unroll
                for (int j = 0; j < NR; j++) {
                    opos[j] = o0 + wave_sum_multi_index<OB>(lane, j);
                    mine[j] = wave_sum_multi_owner<OB>(lane) && opos[j] < n_out;
                }
                phi_late_args(m_stride, pstride, slots_per_output, partial);      // (one scalar wait)
                // where the fold expects this chunk's partials: output-major chunk numbering, or the regular rows' slots (one
                // structure for all outputs); a scalar load behind that wait, in flight until the stores
                if (pslot) slot_ld = uniform_word(pslot + chunk);
                const uint32_t ostride = pslot ? (uint32_t)uniform_value_here(slots_per_output) : ncpo;
#pragma unroll
                for (int j = 0; j < NR; j++) opos[j] *= ostride;
                phi_issue_point();
            }
        }
        const double m0 = mc[cc.x], m1 = mc[cc.y], m2 = mc[cc.z], m3 = mc[cc.w];
        amax = fmax(fmax(amax, fmax(fabs(m0), fabs(m1))), fmax(fabs(m2), fabs(m3)));
#pragma unroll
        for (int oo = 0; oo < OB; oo++) {
            s[oo] = fma(v01[oo].x, m0, s[oo]);
            s[oo] = fma(v01[oo].y, m1, s[oo]);
            s[oo] = fma(v23[oo].x, m2, s[oo]);
            s[oo] = fma(v23[oo].y, m3, s[oo]);
        }
        vo += 2048u; co += (uint32_t)(256 * sizeof(COLT));
    };
    sweep(std::true_type());
    int64_t pdone = 0;      // candidates' partials in front of this one, in bytes
    uint32_t it = 1;
    for (int c = 0;;) {
        for (; it < iters; it++) sweep(std::false_type());
        double t[NR];
        wave_sum_multi<OB>(s, t);
        amax = wave_max_dpp(amax);
        const uint32_t slot = pslot ? (uint32_t)uniform_value_here(slot_ld) : chunk;
        char *pc = reinterpret_cast<char *>(uniform_value_here(partial)) + pdone;
#pragma unroll
        for (int j = 0; j < NR; j++)
            if (mine[j]) store_partial(pc + (opos[j] + slot) * 16u, t[j], amax);
        if (++c >= n_cand) break;
        mc += uniform_value_here(m_stride);      // (not hoisted in front of the loop, where they would be waited for)
        pdone += uniform_value_here(pstride) * (int64_t)sizeof(double2);
        // (the next candidate's offsets taken as they are here: a chunk of one 256-block has the same columns for every candidate,
        //  and their load is not to be moved in front of the loops)
#pragma unroll
        for (int oo = 0; oo < OB; oo++) s[oo] = 0.0;
        amax = 0.0; it = 0;
        vo = lane_value_here(lane * 32u); co = lane_value_here(lane * (uint32_t)(4 * sizeof(COLT)));
    }
}

// fused: fold chunk partials + solve.  grid = (n_out, n_cand), block = fold_threads (fold) -> wavefront 0 (solve).
// want_v: bit0 = also produce v (gradient wanted); bit1 / bit2 = diagnostics (fold only / solve twice)
// that the library does not set.
// The gate of a launch whose tail may REWRITE that gate (the line-search decision's enable output is the same word): it is read
// once per workgroup and handed to every thread through LDS, so a workgroup is on or off as a whole -- a wavefront that read
// the word after the decision's store could otherwise run the tile code on LDS its solving wavefront never filled.
__device__ __forceinline__ bool gate_closed(const int32_t *gate, int *s_closed)
{
    if (!gate) return false;
    if (threadIdx.x == 0) *s_closed = __hip_atomic_load(gate, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT) == 0 ? 1 : 0;
    __syncthreads();
    return *s_closed != 0;
}

template <int NT>
__global__ __launch_bounds__(fold_threads(NT)) void k_solve_from_chunks(int N, int n_out, const RowDesc *__restrict__ rows, int nsym, FoldReg reg,
                                                           const double2 *__restrict__ partial, int64_t n_chunks,
                                                           double delta, int want_v, double *__restrict__ var,
                                                           double *__restrict__ v, int32_t *__restrict__ status,
                                                           const int32_t *__restrict__ gate, double *__restrict__ spg_state, int last_slot, int32_t *__restrict__ spg_enable,
                                                           unsigned int *__restrict__ ticket)
{
    __shared__ SolveLds<NT> lds;
    __shared__ double spg_ls[SPG_STATE_DOUBLES];
    __shared__ int s_closed;
    // everything in front of the fold's first load arrives in one batch (kernarg_now, common.hpp)
    kernarg_now(N, n_out, rows, nsym, reg.Cd, reg.Co, reg.rank_ab, partial, n_chunks, gate, spg_state);
    const int o = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    if (gate_closed(gate, &s_closed)) {   // device-side predication (SPG line-search slots)
        // the line-search decision still has to close the slot (it sets the gate of the finishing launches on the last one).
        // Its enable output IS the gate, so it may only write once every workgroup of this launch has read the gate: they take a
        // ticket of their own (ticket[16]) and the last one to arrive decides.
        if (spg_state && tid < WAVE && spg_closed_last(ticket + 16, gridDim.x * gridDim.y, tid))
            spg_decide_wave(spg_state, var, status, n_out, last_slot, spg_enable, spg_ls, tid);
        return;
    }
    SpgPrefetch pf;
    if (spg_state && tid < WAVE) spg_prefetch_state(spg_state, tid, pf);   // in flight during the fold (see spg_state.hpp)
    if (N < NT) { clear_pads(lds, N, tid, fold_threads(NT)); __syncthreads(); }   // uniform; every real entry is written by the fold
    fold_rows(lds, N, rows, o, nsym, partial + (int64_t)c * n_chunks, tid, fold_threads(NT), reg);
    __syncthreads();
    if (tid >= WAVE) return;   // single wavefront from here on
    const int lane = tid;
    if (spg_state) spg_prefetch_parts(pf, lane);                           // in flight during the elimination
    const int64_t e = (int64_t)c * n_out + o;
    if (want_v & 2) {   // diagnostics: fold only (timing experiments)
        if (lane == 0) { var[e] = lds.at(0, 0); status[e] = 0; }
        return;
    }
    const double am = (lane < N) ? lds.amax[lane] : 0.0;
    const bool big = __ballot(am >= 0.05) != 0ull;   // max |m| >= 0.05 (misc.py:464)
    const int reps = (want_v & 4) ? 2 : 1;   // diagnostics: run the solve twice
    double V_mine = 0.0;
    int32_t st_mine = 0;
    for (int rep = 0; rep < reps; rep++)
        solve_wave<NT>(lds, N, delta, am > 1.0e-6, am > 0.0, big, (want_v & 1) != 0, &V_mine, v + e * N, &st_mine, lane);
    if (lane == 0) { var[e] = V_mine; status[e] = st_mine; }
    if (spg_state) {
        // line-search decision fused into the tail (single candidate): every output's workgroup publishes V and status, takes a
        // ticket, and the LAST one to arrive evaluates the objective of the trial point and decides -- one launch and one kernel
        // boundary less per slot.  Publication: stores drained, agent-scope release, then the ticket (relaxed agent atomic);
        // the last arriver acquires before it reads the other outputs' values (MI355X_MICROARCH.md, inter-workgroup visibility).
        int last = 0;
        if (n_out == 1) {   // single output: nobody to wait for, V and status stay in lane 0's registers
            spg_decide_wave(spg_state, var, status, n_out, last_slot, spg_enable, spg_ls, lane, pf, true, V_mine, st_mine);
            return;
        }
        if (lane == 0) {
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
            asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
            const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            last = (t == (unsigned int)(n_out - 1)) ? 1 : 0;
            if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);      // ready for the next launch
        }
        last = __builtin_amdgcn_readfirstlane(last);
        if (last) {
            __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
            spg_decide_wave(spg_state, var, status, n_out, last_slot, spg_enable, spg_ls, lane, pf);
        }
    }
}

// multi-GPU path, phase A tail: fold chunk partials into an all-reduce-able record.
template <int NT>
__global__ __launch_bounds__(fold_threads(NT)) void k_fold_to_record(int N, int n_out, const RowDesc *__restrict__ rows, int nsym, FoldReg reg,
                                                        const double2 *__restrict__ partial, int64_t n_chunks,
                                                        double *__restrict__ rec)
{
    __shared__ SolveLds<NT> lds;
    kernarg_now(N, n_out, rows, nsym, reg.Cd, reg.Co, reg.rank_ab, partial, n_chunks, rec);      // one batch (common.hpp)
    const int o = blockIdx.x, c = blockIdx.y, tid = threadIdx.x;
    fold_rows(lds, N, rows, o, nsym, partial + (int64_t)c * n_chunks, tid, fold_threads(NT), reg);
    __syncthreads();
    const int reclen = N * N + 2 * N + 1;
    double *r = rec + ((int64_t)c * n_out + o) * reclen;
    for (int t = tid; t < N * N; t += fold_threads(NT)) r[t] = lds.at(t / N, t % N);
    if (tid >= WAVE) return;
    const double am = (tid < N) ? lds.amax[tid] : 0.0;
    if (tid < N) { r[N * N + tid] = (am > 1.0e-6) ? 1.0 : 0.0; r[N * N + N + tid] = (am > 0.0) ? 1.0 : 0.0; }
    const double big = wave_max(am);
    if (tid == 0) r[N * N + 2 * N] = (big >= 0.05) ? 1.0 : 0.0;
}

// multi-GPU path, phase B: solve from an (all-reduced) record.  block = 64.
template <int NT>
__global__ __launch_bounds__(64) void k_solve_from_record(int N, int n_out, const double *__restrict__ rec,
                                                          double delta, int want_v, double *__restrict__ var,
                                                          double *__restrict__ v, int32_t *__restrict__ status)
{
    __shared__ SolveLds<NT> lds;
    const int o = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const int reclen = N * N + 2 * N + 1;
    const double *r = rec + ((int64_t)c * n_out + o) * reclen;
    clear_pads(lds, N, lane, WAVE);
    __syncthreads();
    for (int t = lane; t < N * N; t += WAVE) lds.at(t / N, t % N) = r[t];
    __syncthreads();
    const bool s1 = lane < N && r[N * N + lane] > 0.0;
    const bool s2 = lane < N && r[N * N + N + lane] > 0.0;
    const bool big = r[N * N + 2 * N] > 0.0;
    const int64_t e = (int64_t)c * n_out + o;
    solve_wave<NT>(lds, N, delta, s1, s2, big, (want_v & 1) != 0, var + e, v + e * N, status + e, lane);
}

// Rare path (bluest_plan_solve_pinv): what the reference's variance_GH returns when the restricted Phi is rank-deficient --
// numpy pinv, i.e. eigenvalues not larger than 1e-15 * max|lambda| dropped (misc.py:487,490).  One wavefront per (candidate,
// output), lane r = row r; cyclic Jacobi exactly as sym_pinv_jacobi (mirrors.hip) does it per group, with the matrix and the
// eigenvectors in LDS because the size is a run-time value here.  Models outside the index set keep zero rows / columns: their
// eigenvalues are zero and drop out, so the pseudo-inverse of the padded matrix is the padded pseudo-inverse.
__device__ __forceinline__ void jacobi_pinv_lds(double *A, double *Q, int N, int LD, int lane)
{
    for (int sweep = 0; sweep < 60; sweep++) {
        int rotated = 0;
        for (int p = 0; p < N - 1; p++)
            for (int q = p + 1; q < N; q++) {
                const double apq = A[p * LD + q], app = A[p * LD + p], aqq = A[q * LD + q];      // same address in every lane
                if (!(fabs(apq) > 1.0e-18 * sqrt(fabs(app * aqq)))) continue;                    // uniform (also skips zeros / NaN)
                rotated = 1;
                const double theta = (aqq - app) / (2.0 * apq);
                const double t = (theta >= 0 ? 1.0 : -1.0) / (fabs(theta) + sqrt(theta * theta + 1.0));
                const double c = 1.0 / sqrt(t * t + 1.0), sn = t * c;
                if (lane < N) {
                    const double arp = A[lane * LD + p], arq = A[lane * LD + q];
                    A[lane * LD + p] = c * arp - sn * arq;
                    A[lane * LD + q] = sn * arp + c * arq;
                    const double vrp = Q[lane * LD + p], vrq = Q[lane * LD + q];
                    Q[lane * LD + p] = c * vrp - sn * vrq;
                    Q[lane * LD + q] = sn * vrp + c * vrq;
                }
                wave_lds_sync();
                if (lane < N) {
                    const double apr = A[p * LD + lane], aqr = A[q * LD + lane];
                    A[p * LD + lane] = c * apr - sn * aqr;
                    A[q * LD + lane] = sn * apr + c * aqr;
                }
                wave_lds_sync();
            }
        if (!rotated) break;
    }
}

__global__ __launch_bounds__(64) void k_pinv_from_record(int N, int n_out, const double *__restrict__ rec, double delta,
                                                         double *__restrict__ var, double *__restrict__ v,
                                                         int32_t *__restrict__ status)
{
    extern __shared__ double pinv_sm[];
    const int LD = N + 1;
    double *A = pinv_sm, *Q = pinv_sm + N * LD;
    const int o = blockIdx.x, c = blockIdx.y, lane = threadIdx.x;
    const int reclen = N * N + 2 * N + 1;
    const double *r = rec + ((int64_t)c * n_out + o) * reclen;
    const int64_t e = (int64_t)c * n_out + o;
    const bool s1 = lane < N && r[N * N + lane] > 0.0;
    const bool s2 = lane < N && r[N * N + N + lane] > 0.0;
    const bool big = r[N * N + 2 * N] > 0.0;
    const unsigned long long mask1 = __ballot(s1);
    const unsigned long long mask2 = (delta != 0.0) ? __ballot(lane < N) : __ballot(s2);
    int st = BLUEST_EVAL_OK;
    double V = 0.0, vmine = 0.0;
    if (!big) { st = BLUEST_EVAL_INF; V = INFINITY; }
    else if (mask1 == 0ull) { st = BLUEST_EVAL_NO_MODEL0; V = NAN; }
    else {
        if (!(mask1 & 1ull)) st = BLUEST_EVAL_NO_MODEL0;
        const int npass = (mask1 == mask2) ? 1 : 2;
        for (int pass = 0; pass < npass; pass++) {
            const unsigned long long mask = pass == 0 ? mask1 : mask2;
            if (lane < N)
                for (int j = 0; j < N; j++) {
                    const bool in = ((mask >> lane) & 1ull) && ((mask >> j) & 1ull);
                    A[lane * LD + j] = in ? 0.5 * (r[lane * N + j] + r[j * N + lane]) + (lane == j ? delta : 0.0) : 0.0;
                    Q[lane * LD + j] = lane == j ? 1.0 : 0.0;
                }
            // scaled to ordinary size by a power of two where max|a| lies outside 2^-256 .. 2^256 (pow2_exponent, common.hpp):
            // the rotation threshold of jacobi_pinv_lds is a product of two entries, inf from 2^512 on (nothing rotates) and 0
            // below 2^-537 (nothing is skipped)
            double rmax = 0.0;
            if (lane < N)
                for (int j = 0; j < N; j++) rmax = fmax(rmax, fabs(A[lane * LD + j]));
            const int sh = pow2_exponent(wave_max(rmax));
            if (lane < N)
                for (int j = 0; j < N; j++) A[lane * LD + j] = ldexp(A[lane * LD + j], -sh);
            wave_lds_sync();
            jacobi_pinv_lds(A, Q, N, LD, lane);
            const double w = lane < N ? A[lane * LD + lane] : 0.0;
            const double cut = 1.0e-15 * wave_max(fabs(w));
            if (lane < N) A[lane * LD + lane] = fabs(w) > cut ? 1.0 / w : 0.0;        // the diagonal now holds 1/lambda or 0
            wave_lds_sync();
            const int t = __ffsll((long long)mask1) - 1;       // first row of the restricted matrix (model 0 unless unsampled)
            if (pass == 0) {
                double acc = 0.0;
                for (int ee = 0; ee < N; ee++) acc += Q[t * LD + ee] * A[ee * LD + ee] * Q[t * LD + ee];
                V = ldexp(acc, -sh);
            }
            if (pass == npass - 1) {                           // row 0 of pinv(Phi): zero when model 0 is outside the support
                double acc = 0.0;
                if (lane < N && (mask2 & 1ull))
                    for (int ee = 0; ee < N; ee++) acc += Q[0 * LD + ee] * A[ee * LD + ee] * Q[lane * LD + ee];
                vmine = ldexp(acc, -sh);
            }
            wave_lds_sync();
        }
    }
    if (lane < N) v[e * N + lane] = vmine;
    if (lane == 0) { var[e] = V; status[e] = st; }
}

// KU = largest group size with a fully unrolled register path in this instantiation (the host picks the smallest
// KU covering the plan, so the common small-k plans keep a small register footprint)
template <int KU>
__global__ __launch_bounds__(256) void k_grad_tiles(const TileDesc *__restrict__ tiles, int64_t n_tiles,
                                                    const double *__restrict__ tvals, const double *__restrict__ v,
                                                    const int32_t *__restrict__ status, int N, int n_out, int n_cand,
                                                    double *__restrict__ grad, int64_t grad_stride,
                                                    const int32_t *__restrict__ gate)
{
    if (gate && *gate == 0) return;   // device-side predication (SPG line-search slots)
    const int64_t t = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int lane = threadIdx.x & 63;
    if (t >= n_tiles) return;
    const TileDesc td = tiles[t];
#define GT(KK) case KK: if (KK <= KU) { grad_tile<(KK <= KU ? KK : 1)>(td, tvals, v, status, N, n_out, n_cand, grad, grad_stride, lane); break; }
    switch (td.k) {
        GT(1) GT(2) GT(3) GT(4) GT(5) GT(6) GT(7) GT(8) GT(9) GT(10) GT(11) GT(12)
        default: grad_tile_generic(td, tvals, v, status, N, n_out, n_cand, grad, grad_stride, lane);
    }
#undef GT
}

// Fused solve + gradient pass (single candidate): every workgroup owns 4 tiles of ONE output, folds that output's chunk
// partials and factorises Phi itself (redundantly with the other workgroups of the output -- ~2.5 us of one wavefront,
// no inter-workgroup hand-off, so nothing to synchronise), then its 4 wavefronts evaluate their tiles with v read from
// LDS.  Saves one dependent launch per evaluation.  The tile list is padded so that no workgroup straddles two outputs.
// tiles per workgroup of the fused kernel: wavefront 0 solves, wavefronts 1..TPB own one tile each.  15 (1024 threads,
// 128 VGPRs) while the register-resident matrix (2 NT VGPRs) and tile (KU (KU+1) + KU VGPRs) fit, else 7 (512 threads, 256 VGPRs)
__host__ __device__ constexpr int fused_tpb(int NT, int KU) { return (NT <= 26 && KU <= 8) ? 15 : 7; }
using SolveGradKuSet = InstSet<5, 6, 8, 12>;     // KU of k_solve_grad
using GradTilesKuSet = InstSet<5, 8, 12>;        // KU of k_grad_tiles
using PhiObSet = InstSet<2, 4, 8>;               // OB of k_phi_chunks_shared (phi_ob)
template <class F> static void solve_grad_ku_dispatch(int kmax, F &&launch) { SolveGradKuSet::dispatch(kmax, launch); }
// Arguments: the first 14 dwords arrive in scalar registers with the wavefront (kernarg preload, see the chunk kernels), and they
// hold what the fold needs in front of its first load: partial, the members of the FoldReg, rows and tiles (the descriptor fold's
// and the ragged grid's first loads), N and nsym in one word (n_nsym = N | nsym << 8; bluest_plan_finalize checks N <= 64 and
// nsym <= 2080), bpo and a flags word.  rec, gate and spg_state are null in the plain step: the flags say which one is there, and
// a pointer is loaded inside the branch that uses it.  What the solving wavefront and the tile stream need behind the barrier is
// requested in front of the fold and waited for behind the issue of its first loads (the hook given to fold_rows).
constexpr uint32_t SG_HAS_REC = 1u, SG_HAS_GATE = 2u, SG_HAS_SPG = 4u;
template <int NT, int KU>
__global__ __launch_bounds__(64 * (fused_tpb(NT, KU) + 1)) void k_solve_grad(const double2 *__restrict__ partial, const uint16_t *__restrict__ rank_ab,
                                                    const RowDesc *__restrict__ rows, const TileDesc *__restrict__ tiles,
                                                    uint32_t n_nsym, int Cd, int Co, int bpo, uint32_t flags,
                                                    int n_out_arg, int tpb_arg, int tile_nt, const double *__restrict__ rec_arg, double delta,
                                                    const double *__restrict__ tvals,
                                                    double *__restrict__ var, double *__restrict__ v_ws,
                                                    int32_t *__restrict__ status, double *__restrict__ grad,
                                                    const int32_t *__restrict__ gate, double *__restrict__ spg_state_arg, int last_slot,
                                                    int32_t *__restrict__ spg_enable, unsigned int *__restrict__ ticket, const MaTail ma)
{
    constexpr int FUSED_TPB = fused_tpb(NT, KU);
    constexpr int NTHREADS = 64 * (FUSED_TPB + 1);
    constexpr int PU = tile_pairs(KU);
    __shared__ SolveLds<NT> lds;
    __shared__ double spg_ls[SPG_STATE_DOUBLES];
    const int N = (int)(n_nsym & 0xffu), nsym = (int)(n_nsym >> 8);
    const FoldReg reg{Cd, Co, rank_ab};
    const int tid = threadIdx.x, lane = tid & 63;
    const int wave = __builtin_amdgcn_readfirstlane(tid >> 6);      // (the compiler does not see that tid >> 6 is wave-uniform)
    // which output, and am I its first workgroup: the grid says so when every output has the same number of workgroups (bpo > 0,
    // the usual case: grid = (bpo, n_out), no division), else the first tile's descriptor (grid = (workgroups, 1); one more
    // dependent load in front of the fold, and tpb is waited for in front of it)
    int o, first, wg;
    if (bpo > 0) { o = blockIdx.y; first = blockIdx.x == 0; wg = o * bpo + blockIdx.x; }
    else { wg = blockIdx.x; const TileDesc td0 = tile_desc_uniform(tiles, (int64_t)wg * tpb_arg); o = td0.out; first = (td0.n_valid >> 30) & 1; }
    __shared__ int s_closed;
    double *spg_state = nullptr;
    if (flags & (SG_HAS_GATE | SG_HAS_SPG)) {      // (the line search's launches; the plain step passes this over)
        if (flags & SG_HAS_SPG) spg_state = spg_state_arg;
        if ((flags & SG_HAS_GATE) && gate_closed(gate, &s_closed)) {
            // predicated off; the line-search decision still has to close the slot (see k_solve_from_chunks): the first workgroups
            // of the n_out outputs -- the ones that publish V and status and take the decision ticket when the gate is open -- arrive
            // at a ticket of their own, and the last one decides, so none of THEM can see the gate the decision reopens.  A whole
            // workgroup that is not the first of its output may start after that store and run: it folds the Phi partials of the
            // accepted trial (the predicated-off Phi pass of this slot left them alone), so it rewrites that trial's gradient
            // entries with the same bits.  The other way round (a rejected last slot closes the gate under an open launch) a late
            // workgroup skips gradient entries of a trial nobody uses.
            if (spg_state && first && wave == 0 && spg_closed_last(ticket + 16, (unsigned int)n_out_arg, lane))
                spg_decide_wave(spg_state, var, status, n_out_arg, last_slot, spg_enable, spg_ls, lane);
            return;
        }
    }
    SpgPrefetch pf;
    if (spg_state && first && wave == 0) spg_prefetch_state(spg_state, lane, pf);   // in flight during the fold (spg_state.hpp)
    if (N < NT) { clear_pads(lds, N, tid, NTHREADS); __syncthreads(); }   // uniform; every real entry is written by the fold
    // Phi either folded from this GPU's chunk partials, or (group-sharded plans) taken from the all-reduced record of output o:
    // N*N sums, then the per-model flags "touched with |m| > 1e-6" / "touched at all" and the flag "max|m| >= 0.05" as counts
    const double *rec_o = (flags & SG_HAS_REC) ? rec_arg + (int64_t)o * (N * N + 2 * N + 1) : nullptr;
    if (rec_o) {
        for (int t = tid; t < N * N; t += NTHREADS) lds.at(t / N, t % N) = rec_o[t];
    } else {
        fold_rows<NT>(lds, N, rows, o, nsym, partial, tid, NTHREADS, reg,
                      [&]() { kernarg_now(n_out_arg, tpb_arg, delta, var, v_ws, status); });
    }
    // (what is computed from the late arguments stays behind the fold's loads)
    const int n_out = uniform_value_here(n_out_arg), tpb = uniform_value_here(tpb_arg);
    const int64_t t0 = (int64_t)wg * tpb;      // tpb <= FUSED_TPB tiles per workgroup (wavefronts beyond it only fold)
    // the list is padded to a multiple of FUSED_TPB tiles per output, so every tile of this workgroup belongs to output o
    // (loaded by the tile wavefronts only: the solving wavefront must not wait for a descriptor it does not use; scalar loads, so
    //  k, the offsets and the group count are scalar: the dispatch on k branches, the tile's and the gradient's bases are formed
    //  on the scalar unit and a lane adds a 32-bit offset)
    TileDesc td;
    td.k = 1; td.n_valid = 0; td.val_off = td.grad_off = 0; td.out = (int16_t)o;
    if (wave > 0 && wave <= tpb) td = tile_desc_uniform(tiles, t0 + wave - 1);
    __syncthreads();
    const int k = td.k;
    double2 pr[PU];
    double V_pub = 0.0;      // wavefront 0: V and status of this workgroup's solve (for the single-output decision)
    int32_t st_pub = 0;
    if (wave == 0) {
        if (spg_state && first) spg_prefetch_parts(pf, lane);                       // in flight during the elimination
        bool s1, s2, big;
        if (rec_o) {
            s1 = lane < N && rec_o[N * N + lane] > 0.0;
            s2 = lane < N && rec_o[N * N + N + lane] > 0.0;
            big = rec_o[N * N + 2 * N] > 0.0;
        } else {
            const double am = (lane < N) ? lds.amax[lane] : 0.0;
            s1 = am > 1.0e-6;
            s2 = am > 0.0;
            big = __ballot(am >= 0.05) != 0ull;          // max |m| >= 0.05 (misc.py:464)
        }
        double V = 0.0;
        int32_t st = 0;
        solve_wave<NT>(lds, N, delta, s1, s2, big, true, &V, lds.vout, &st, lane);
        if (lane == 0) { lds.status = st; if (ma.x) lds.scratch[0] = V; }      // (the elimination is done with its scratch)
        V_pub = V; st_pub = st;
        if (first) {   // first workgroup of this output publishes V, status, v
            if (lane == 0) { var[o] = V; status[o] = st; }
            if (lane < N) v_ws[(int64_t)o * N + lane] = lds.vout[lane];
        }
    } else if (k <= KU) {
        // stream the tile into registers while wavefront 0 factorises (after the fold, so these loads do not queue in front of it)
        if (tile_nt) tile_load<PU, true>(pr, tvals + td.val_off, lane, tile_pairs(k));
        else tile_load(pr, tvals + td.val_off, lane, tile_pairs(k));
    }
    __syncthreads();
    if (wave == 0) {
        if (spg_state && first) {
            // SPG line search: the first workgroup of every output has published V and status above; they take a ticket and the
            // last one to arrive decides (same protocol as the tail of k_solve_from_chunks), while the tile wavefronts of all
            // workgroups compute the gradient of this trial point -- it is the one the update needs if the trial is accepted
            int last = 0;
            if (n_out == 1) {   // single output: nobody to wait for, V and status stay in lane 0's registers
                spg_decide_wave(spg_state, var, status, n_out, last_slot, spg_enable, spg_ls, lane, pf, true, V_pub, st_pub);
                return;
            }
            if (lane == 0) {
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                __builtin_amdgcn_fence(__ATOMIC_RELEASE, "agent");
                asm volatile("s_waitcnt vmcnt(0)" ::: "memory");
                const unsigned int t = __hip_atomic_fetch_add(ticket, 1u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
                last = (t == (unsigned int)(n_out - 1)) ? 1 : 0;
                if (last) __hip_atomic_store(ticket, 0u, __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            }
            last = __builtin_amdgcn_readfirstlane(last);
            if (last) {
                __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "agent");
                spg_decide_wave(spg_state, var, status, n_out, last_slot, spg_enable, spg_ls, lane, pf);
            }
        }
        return;
    }
    const bool valid = lane < (td.n_valid & 0xffff);
    const bool inf = lds.status == BLUEST_EVAL_INF;
    double *gout = grad + td.grad_off + lane;
    // (single output, phase 1 of the second-order finish: the update itself instead of the gradient -- k_ma_update's arithmetic)
    const bool MA_ON = ma.x != nullptr;
#define GT(KK) case KK: if (KK <= KU) { const double q = tile_form<(KK <= KU ? KK : 1)>(pr, lds.vout);                                          \
        if (valid && !MA_ON) *gout = inf ? INFINITY : -q;                                                                                        \
        else if (valid && lds.status == BLUEST_EVAL_OK) { const int64_t i = td.grad_off + lane; const double so = ma.s[0], cci = ma.cc[i];       \
            const double xn = ma.x[i] * cci * ((1.0 / so) * q) / (lds.scratch[0] / so); ma.x[i] = xn; ma.m[i] = cci * xn; } break; }
    switch (k) {
        GT(1) GT(2) GT(3) GT(4) GT(5) GT(6) GT(7) GT(8) GT(9) GT(10) GT(11) GT(12)
        default: {
            // grad_tile reads v as v[(c*n_out + td.out)*N + model] and status[c*n_out + td.out]: point both at LDS
            const double *vl = lds.vout - (int64_t)td.out * N;
            const int32_t *sl = &lds.status - td.out;
            grad_tile_generic(td, tvals, vl, sl, N, n_out, 1, grad, 0, lane);
        }
    }
#undef GT
}

// out[c][j] = scale[j] * sum_o coef[c][o] * grad_o[c][invmap_o[j]]
__global__ void k_combine_grad(const double *__restrict__ grad, int64_t grad_stride, const int64_t *__restrict__ goff,
                               const int32_t *__restrict__ invmap, int64_t L, int n_out,
                               const double *__restrict__ coef, const double *__restrict__ scale, int n_cand,
                               double *__restrict__ out, int64_t out_stride, const int32_t *__restrict__ gate)
{
    if (gate && *gate == 0) return;   // device-side predication (SPG line-search slots)
    const int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int c = blockIdx.y;
    if (j >= L || c >= n_cand) return;
    double s = 0.0;
    for (int o = 0; o < n_out; o++) {
        const int32_t li = invmap[(int64_t)o * L + j];
        if (li >= 0) s = fma(coef[(int64_t)c * n_out + o], grad[(int64_t)c * grad_stride + goff[o] + li], s);
    }
    out[(int64_t)c * out_stride + j] = scale ? scale[j] * s : s;
}

// ------------------------------------------------------------------------------------------------------
// Part 2 host side: the plan
// ------------------------------------------------------------------------------------------------------
// Device memory of plans comes from a small cache owned by the library: a released block is kept (up to CACHE_CAP bytes) and
// handed to the next request of a similar size.  Measured alternatives: hipMalloc / hipFree of the 45 MB arena cost 10-80 ms
// depending on what else the process holds; HIP's stream-ordered pool (hipMallocAsync) was fast to allocate from but every
// second set-up stalled ~75 ms inside the next null-stream synchronisation while the runtime trimmed and re-mapped the pool.
// Blocks are only recycled after a device synchronisation (plan_release), so no kernel of the previous owner is still running.
#include <map>
#include <unordered_map>
// Blocks belong to the DEVICE they were allocated on: the cache is keyed by (device, size) and a block is only ever handed to a
// request made with the same current device (Plan(device=...) is a public argument; a block of cuda:0 inside a plan of cuda:1
// would be a memory fault, not an error code).
struct BlockInfo { size_t size; int device; };
static std::mutex g_cache_mutex;
static std::multimap<std::pair<int, size_t>, void *> g_cache;   // free blocks by (device, size)
static std::unordered_map<void *, BlockInfo> g_block_info;      // every block handed out or cached
static size_t g_cache_bytes = 0;
static const size_t CACHE_CAP = 3ull << 30;

hipError_t pool_alloc(void **p, size_t bytes)
{
    size_t want = (std::max<size_t>(bytes, 1) + 0x3ffff) & ~(size_t)0x3ffff;            // 256 KiB granules
    if (want <= (8u << 20)) {                  // small requests (restricted plans of the solver): power-of-two size classes, so
        size_t cls = 512u << 10;               // that the next plan of a slightly different size reuses the block
        while (cls < want) cls <<= 1;
        want = cls;
    }
    int dev = 0;
    hipError_t e = hipGetDevice(&dev);
    if (e != hipSuccess) return e;
    {
        std::lock_guard<std::mutex> lock(g_cache_mutex);
        auto it = g_cache.lower_bound(std::make_pair(dev, want));
        if (it != g_cache.end() && it->first.first == dev && it->first.second <= 2 * want + (1u << 20)) {
            *p = it->second;
            g_cache_bytes -= it->first.second;
            g_cache.erase(it);
            return hipSuccess;
        }
    }
    e = hipMalloc(p, want);
    if (e != hipSuccess) {       // out of memory: give this device's cached blocks back and try once more
        (void)hipGetLastError();
        std::vector<void *> drop;
        {
            std::lock_guard<std::mutex> lock(g_cache_mutex);
            for (auto it = g_cache.begin(); it != g_cache.end();) {
                if (it->first.first != dev) { ++it; continue; }
                drop.push_back(it->second);
                g_cache_bytes -= it->first.second;
                g_block_info.erase(it->second);
                it = g_cache.erase(it);
            }
        }
        for (void *q : drop) (void)hipFree(q);
        e = hipMalloc(p, want);
    }
    if (e == hipSuccess) {
        std::lock_guard<std::mutex> lock(g_cache_mutex);
        g_block_info[*p] = BlockInfo{want, dev};
    }
    return e;
}
// recycle = false: the block is handed back to the runtime instead of the cache (error paths: nothing that a faulted or
// half-finished sequence touched is given to the next plan)
hipError_t pool_free(void *p, bool recycle)
{
    {
        std::lock_guard<std::mutex> lock(g_cache_mutex);
        auto it = g_block_info.find(p);
        if (it == g_block_info.end()) return hipFree(p);
        const BlockInfo bi = it->second;
        if (recycle && g_cache_bytes + bi.size <= CACHE_CAP) {
            g_cache.emplace(std::make_pair(bi.device, bi.size), p);
            g_cache_bytes += bi.size;
            return hipSuccess;
        }
        g_block_info.erase(it);
    }
    return hipFree(p);
}

static void output_release(OutputDesc &od)
{
    if (od.d_invcov) (void)pool_free(od.d_invcov);
    if (od.d_groups && od.owns_groups) (void)pool_free(od.d_groups);
    od.d_invcov = nullptr; od.d_groups = nullptr;
}

static void plan_free_device(bluest_plan_s *p)
{
    mf_release(p);
    if (p->d_arena) (void)pool_free(p->d_arena);
    if (p->d_scratch) (void)pool_free(p->d_scratch);
    if (p->d_master) (void)pool_free(p->d_master);
    p->d_arena = p->d_scratch = p->d_master = nullptr;
    p->master_bytes = 0;
    for (auto &od : p->outs) output_release(od);
}

extern "C" int bluest_plan_create(bluest_plan_t *plan, int n_models, int64_t L_global)
{
    if (!plan) return fail(BLUEST_ERR_ARG, "plan is NULL");
    if (n_models <= 0 || n_models > BLUEST_MAX_MODELS)
        return fail(BLUEST_ERR_ARG, "n_models=%d out of range (1..%d)", n_models, BLUEST_MAX_MODELS);
    if (L_global <= 0 || L_global > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "L_global=%lld out of range", (long long)L_global);
    int rc = require_gpu(); if (rc) return rc;
    bluest_plan_s *p = new bluest_plan_s();
    p->N = n_models;
    p->L = L_global;
    if (hipGetDevice(&p->device) != hipSuccess) { delete p; return fail(BLUEST_ERR_HIP, "hipGetDevice failed"); }
    *plan = p;
    return BLUEST_OK;
}

// Plan lifetime vs stream capture: freeing device memory (hipFreeAsync on the null stream) while ANOTHER stream of the process
// is being captured into a hipGraph invalidates that capture (hipErrorStreamCaptureInvalidated).  A host language with a
// garbage collector or reference counting can drop a plan at any point, so the library does not rely on the caller's timing:
// between bluest_capture_guard(1) and bluest_capture_guard(0) destroyed plans are parked and released when the guard closes.
static std::mutex g_defer_mutex;
static int g_capture_depth = 0;
static std::vector<bluest_plan_s *> g_deferred;

static void plan_release(bluest_plan_s *p)
{
    DeviceScope scope(p->device);       // the caller may be on another device (a destructor runs wherever the last reference dies)
    (void)hipDeviceSynchronize();       // the blocks go back to the cache: nothing of this plan may still be running
    plan_free_device(p);
    delete p;
}

extern "C" int bluest_capture_guard(int on)
{
    std::vector<bluest_plan_s *> drain;
    {
        std::lock_guard<std::mutex> lock(g_defer_mutex);
        if (on) { g_capture_depth++; return BLUEST_OK; }
        if (g_capture_depth > 0) g_capture_depth--;
        if (g_capture_depth == 0) drain.swap(g_deferred);
    }
    for (bluest_plan_s *p : drain) plan_release(p);
    return BLUEST_OK;
}

extern "C" int bluest_deferred_plans(int *count)
{
    if (!count) return fail(BLUEST_ERR_ARG, "count is NULL");
    std::lock_guard<std::mutex> lock(g_defer_mutex);
    *count = (int)g_deferred.size();
    return BLUEST_OK;
}

extern "C" int bluest_plan_destroy(bluest_plan_t plan)
{
    if (!plan) return BLUEST_OK;
    {
        std::lock_guard<std::mutex> lock(g_defer_mutex);
        if (g_capture_depth > 0) { g_deferred.push_back(plan); return BLUEST_OK; }
    }
    plan_release(plan);
    return BLUEST_OK;
}

static int plan_add_common(bluest_plan_t plan, int K, const int64_t *sizes, const int64_t *groups, const int64_t *mapping,
                           OutputDesc &od)
{
    if (!plan) return fail(BLUEST_ERR_ARG, "plan is NULL");
    if (plan->finalized) return fail(BLUEST_ERR_STATE, "plan already finalized");
    if (K <= 0 || K > BLUEST_MAX_GROUP) return fail(BLUEST_ERR_ARG, "K=%d out of range (1..%d): groups hold at most BLUEST_MAX_GROUP = %d models", K, BLUEST_MAX_GROUP, BLUEST_MAX_GROUP);
    if (!sizes || !groups) return fail(BLUEST_ERR_ARG, "null pointer");
    if ((int)plan->outs.size() >= 32767) return fail(BLUEST_ERR_ARG, "too many outputs");
    od.K = K;
    od.sizes.assign(sizes, sizes + K);
    int64_t L_o = 0, ng = 0;
    for (int k = 1; k <= K; k++) {
        if (sizes[k - 1] < 0) return fail(BLUEST_ERR_ARG, "negative size");
        L_o += sizes[k - 1];
        ng += sizes[k - 1] * k;
    }
    if (L_o <= 0) return fail(BLUEST_ERR_ARG, "output has no groups");
    od.L_o = L_o;
    od.groups.assign(groups, groups + ng);
    for (int64_t t = 0; t < ng; t++)
        if (groups[t] < 0 || groups[t] >= plan->N) return fail(BLUEST_ERR_ARG, "model index %lld out of range", (long long)groups[t]);
    if (mapping) {
        od.mapping.assign(mapping, mapping + L_o);
        for (int64_t t = 0; t < L_o; t++)
            if (mapping[t] < 0 || mapping[t] >= plan->L) return fail(BLUEST_ERR_ARG, "mapping index %lld out of range", (long long)mapping[t]);
    } else {
        if (L_o != plan->L) return fail(BLUEST_ERR_ARG, "identity mapping needs L_o == L_global (%lld vs %lld)", (long long)L_o, (long long)plan->L);
        od.mapping.resize(L_o);
        for (int64_t t = 0; t < L_o; t++) od.mapping[t] = t;
    }
    return BLUEST_OK;
}

// device copies of one output's inputs: the group list (shared with output 0 when identical) and room for its inverses
static int output_to_device(bluest_plan_t plan, OutputDesc &od)
{
    int64_t ni = 0, ng = 0;
    for (int k = 1; k <= od.K; k++) { ni += od.sizes[k - 1] * k * k; ng += od.sizes[k - 1] * k; }
    od.n_inv = ni;
    HIP_TRY(pool_alloc((void **)&od.d_invcov, (size_t)std::max<int64_t>(ni, 1) * sizeof(double)));
    if (!plan->outs.empty() && plan->outs[0].groups == od.groups) {
        od.d_groups = plan->outs[0].d_groups;
        od.owns_groups = false;
    } else {
        HIP_TRY(pool_alloc((void **)&od.d_groups, (size_t)std::max<int64_t>(ng, 1)));
        od.owns_groups = true;
        std::vector<uint8_t> narrow((size_t)ng);
        for (int64_t t = 0; t < ng; t++) narrow[(size_t)t] = (uint8_t)od.groups[(size_t)t];   // validated: 0 <= index < N <= 64
        HIP_TRY(hipMemcpy(od.d_groups, narrow.data(), (size_t)ng, hipMemcpyHostToDevice));
    }
    return BLUEST_OK;
}

extern "C" int bluest_plan_add_output(bluest_plan_t plan, int K, const int64_t *sizes, const int64_t *groups,
                                      const double *invcovs, const int64_t *mapping)
{
    OutputDesc od;
    PhaseTimer timer("plan_add_output");
    int rc = plan_add_common(plan, K, sizes, groups, mapping, od);
    if (rc) return rc;
    if (!invcovs) return fail(BLUEST_ERR_ARG, "invcovs is NULL");
    timer.lap("copy groups / mapping");
    if ((rc = output_to_device(plan, od))) { output_release(od); return rc; }
    timer.lap("device buffers + groups upload");
    hipError_t e = hipMemcpy(od.d_invcov, invcovs, (size_t)od.n_inv * sizeof(double), hipMemcpyHostToDevice);
    timer.lap("H2D inverses");
    if (e != hipSuccess) { output_release(od); HIP_TRY(e); }
    plan->outs.push_back(std::move(od));
    return BLUEST_OK;
}

extern "C" int bluest_plan_add_output_cov(bluest_plan_t plan, const double *C, int K, const int64_t *sizes,
                                          const int64_t *groups, const int64_t *mapping, double *invcovs_out)
{
    OutputDesc od;
    PhaseTimer timer("plan_add_output_cov");
    int rc = plan_add_common(plan, K, sizes, groups, mapping, od);
    if (rc) return rc;
    timer.lap("copy groups / mapping");
    if (!C) return fail(BLUEST_ERR_ARG, "C is NULL");
    const int N = plan->N;
    if ((rc = output_to_device(plan, od))) { output_release(od); return rc; }
    timer.lap("device buffers + groups upload");
    // the covariance goes through a small scratch that is reused across outputs (freed by finalize)
    const size_t need = (size_t)N * N * sizeof(double);
    if (need > plan->scratch_bytes) {
        if (plan->d_scratch) (void)pool_free(plan->d_scratch);
        plan->d_scratch = nullptr; plan->scratch_bytes = 0;
        hipError_t ea = pool_alloc(&plan->d_scratch, need);
        if (ea != hipSuccess) { output_release(od); HIP_TRY(ea); }
        plan->scratch_bytes = need;
    }
    double *dC = reinterpret_cast<double *>(plan->d_scratch);
    hipError_t e = hipMemcpy(dC, C, need, hipMemcpyHostToDevice);     // synchronous: the scratch may be rewritten by the next call
    timer.lap("H2D covariance");
    if (e == hipSuccess) {
        int64_t go = 0, io = 0;
        for (int k = 1; k <= K && rc == BLUEST_OK; k++) {
            const int64_t Lk = sizes[k - 1];
            if (Lk > 0) rc = launch_group_pinv_u8(dC, N, k, Lk, od.d_groups + go, od.d_invcov + io, 0);
            go += Lk * k; io += Lk * k * k;
        }
        // the next output's covariance upload overwrites dC: wait for the kernels (they take ~0.1 ms; the inverses stay on the device)
        od.h_C.assign(C, C + (size_t)N * N);      // the covariance itself is kept (5 KB): the matrix-free evaluation recomputes the inverses from it
        if (rc == BLUEST_OK) e = hipStreamSynchronize(0);
        if (rc == BLUEST_OK && e == hipSuccess && invcovs_out)
            e = hipMemcpy(invcovs_out, od.d_invcov, (size_t)od.n_inv * sizeof(double), hipMemcpyDeviceToHost);
    }
    timer.lap("pseudo-inverse kernels");
    if (rc) { output_release(od); return rc; }
    if (e != hipSuccess) { output_release(od); HIP_TRY(e); }
    plan->outs.push_back(std::move(od));
    return BLUEST_OK;
}

// reference-layout inverses of output o back to the host (lazily: the plan itself never needs them there)
extern "C" int bluest_plan_get_invcovs(bluest_plan_t plan, int output, double *invcovs_out)
{
    if (!plan || !invcovs_out) return fail(BLUEST_ERR_ARG, "null pointer");
    if (output < 0 || output >= (int)plan->outs.size()) return fail(BLUEST_ERR_ARG, "output %d out of range", output);
    const OutputDesc &od = plan->outs[output];
    HIP_TRY(hipMemcpy(invcovs_out, od.d_invcov, (size_t)od.n_inv * sizeof(double), hipMemcpyDeviceToHost));
    return BLUEST_OK;
}

// inverses of SOME groups of output o (local indices, any order): gathered on the device, one small copy back.
// out receives the k x k blocks one after the other (k = size of each requested group).
__global__ void k_gather_blocks(const double *__restrict__ ic, const int64_t *__restrict__ src_off, const int64_t *__restrict__ dst_off,
                                const int32_t *__restrict__ kk, int64_t n, double *__restrict__ out)
{
    const int64_t i = blockIdx.x;
    if (i >= n) return;
    const int k2 = kk[i] * kk[i];
    for (int t = threadIdx.x; t < k2; t += blockDim.x) out[dst_off[i] + t] = ic[src_off[i] + t];
}

extern "C" int bluest_plan_gather_invcovs(bluest_plan_t plan, int output, const int64_t *local_idx, int64_t n, double *out)
{
    if (!plan || !local_idx || !out) return fail(BLUEST_ERR_ARG, "null pointer");
    if (output < 0 || output >= (int)plan->outs.size()) return fail(BLUEST_ERR_ARG, "output %d out of range", output);
    if (n <= 0) return BLUEST_OK;
    const OutputDesc &od = plan->outs[output];
    std::vector<int64_t> cum(od.K + 1, 0), ioff(od.K + 1, 0);
    for (int k = 1; k <= od.K; k++) { cum[k] = cum[k - 1] + od.sizes[k - 1]; ioff[k] = ioff[k - 1] + od.sizes[k - 1] * k * k; }
    std::vector<int64_t> src(n), dst(n);
    std::vector<int32_t> kk(n);
    int64_t total = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t li = local_idx[i];
        if (li < 0 || li >= od.L_o) return fail(BLUEST_ERR_ARG, "group index %lld out of range", (long long)li);
        const int k = (int)(std::upper_bound(cum.begin(), cum.end(), li) - cum.begin());
        src[i] = ioff[k - 1] + (li - cum[k - 1]) * k * k;
        dst[i] = total;
        kk[i] = k;
        total += (int64_t)k * k;
    }
    void *d = nullptr;
    const size_t b_off = (size_t)n * sizeof(int64_t), bytes = 2 * b_off + ((size_t)n * sizeof(int32_t) + 7) / 8 * 8 + (size_t)total * sizeof(double);
    HIP_TRY(pool_alloc(&d, bytes));
    int64_t *d_src = (int64_t *)d, *d_dst = d_src + n;
    int32_t *d_k = (int32_t *)(d_dst + n);
    double *d_out = (double *)((char *)d + 2 * b_off + ((size_t)n * sizeof(int32_t) + 7) / 8 * 8);
    hipError_t e = hipMemcpy(d_src, src.data(), b_off, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_dst, dst.data(), b_off, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_k, kk.data(), (size_t)n * sizeof(int32_t), hipMemcpyHostToDevice);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_gather_blocks, dim3((unsigned)n), dim3(64), 0, 0, od.d_invcov, d_src, d_dst, d_k, n, d_out);
        e = hipMemcpy(out, d_out, (size_t)total * sizeof(double), hipMemcpyDeviceToHost);
    }
    (void)pool_free(d);
    HIP_TRY(e);
    return BLUEST_OK;
}

// ---- device-side construction of the two streaming layouts ----------------------------------------------
// The host only decides WHERE things go (a counting sort of the group list by destination row gives every packed-symmetric
// entry its slot in the CSR; tiles are arithmetic); the VALUES never leave the device: they are scattered from the
// reference-layout inverses (pinv output) by the two kernels below, for one (output, group size) at a time.
__global__ __launch_bounds__(256) void k_fill_csr(const double *__restrict__ ic, int k, int64_t Lk, const int32_t *__restrict__ perm,
                                                  double *__restrict__ vals)
{
    const int ne = k * (k + 1) / 2;
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Lk * ne) return;
    const int64_t gi = t / ne;
    int e = (int)(t - gi * ne), j = 0;
    while (e >= k - j) { e -= k - j; j++; }          // e-th entry of the packed upper triangle: row j, column l = j + e
    const int l = j + e;
    const double *b = ic + gi * k * k;
    vals[perm[t]] = (j == l) ? b[j * k + j] : 0.5 * (b[j * k + l] + b[l * k + j]);
}

__global__ __launch_bounds__(256) void k_fill_tiles(const double *__restrict__ ic, const uint8_t *__restrict__ groups, int k, int64_t Lk,
                                                    double *__restrict__ tvals)
{   // one thread per (group, entry or index byte); the tile layout is described at TileDesc (plan.hpp)
    const int ne = tile_ne(k), ni = tile_ni(k), S = tile_slots(k);
    const int64_t t = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (t >= Lk * (ne + k)) return;
    const int64_t gi = t / (ne + k);
    const int r = (int)(t - gi * (ne + k));
    const int64_t tile = gi >> 6;
    const int lane = (int)(gi & 63);
    double *tb = tvals + tile * S * 64;
    if (r < ne) {
        int e = r, j = 0;
        while (e >= k - j) { e -= k - j; j++; }
        const int l = j + e;
        const double *b = ic + gi * k * k;
        tb[tile_slot_off(ni + r, lane)] = (j == l) ? b[j * k + j] : 0.5 * (b[j * k + l] + b[l * k + j]);
    } else {
        const int j = r - ne;
        reinterpret_cast<uint8_t *>(tb + tile_slot_off(j >> 3, lane))[j & 7] = groups[gi * k + j];
    }
}

// the plan's device arrays live in one arena: reserve() collects sizes, then every array is copied to its slot
struct Arena {
    size_t bytes = 0;
    char *base = nullptr;
    size_t reserve(size_t n) { const size_t off = bytes; bytes += (std::max<size_t>(n, 1) + 255) / 256 * 256; return off; }
};
// a host array that is NOT value-initialised (std::vector zero-fills on one thread and touches every page before the worker
// threads do: 4-5 ms for the 64 MB of slots and columns at K_tot = 245 505); every element is written by the layout passes
template <typename T>
struct RawArray {
    std::unique_ptr<T[]> p;
    size_t n;
    explicit RawArray(size_t n_ = 0) : p(new T[std::max<size_t>(n_, 1)]), n(n_) {}
    void reset(size_t n_) { p.reset(new T[std::max<size_t>(n_, 1)]); n = n_; }
    T *data() { return p.get(); }
    const T *data() const { return p.get(); }
    size_t size() const { return n; }
};
template <typename T, class Host>      // Host: std::vector<T> or RawArray<T>
static int upload(Arena &arena, size_t off, T **dst, const Host &src)
{
    *dst = reinterpret_cast<T *>(arena.base + off);
    if (src.size()) HIP_TRY(hipMemcpy(*dst, src.data(), src.size() * sizeof(T), hipMemcpyHostToDevice));
    return BLUEST_OK;
}

// host-side layout construction on up to 16 worker threads
static int host_threads()
{
    const unsigned hw = std::thread::hardware_concurrency();
    return (int)std::max(1u, std::min<unsigned>(hw ? hw : 1u, 16u));
}
template <class F>
static void parallel_items(int n_items, F fn)
{
    const int nt = std::min(n_items, host_threads());
    if (nt <= 1) { for (int i = 0; i < n_items; i++) fn(i); return; }
    std::atomic<int> next{0};
    std::vector<std::thread> workers;
    for (int t = 0; t < nt; t++)
        workers.emplace_back([&]() { for (;;) { const int i = next++; if (i >= n_items) break; fn(i); } });
    for (auto &w : workers) w.join();
}

// position of the packed-symmetric pair (a, b), a <= b, among the N (N + 1) / 2 rows of the Phi layout
static inline int sym_row(int N, int a, int b) { return a * N - a * (a - 1) / 2 + (b - a); }

// what the steps of bluest_plan_finalize hand to one another (host side; the plan keeps only what its launches read)
struct PlanLayout {
    int n_struct;                                       // distinct group structures (1 when the outputs share theirs)
    std::vector<TileDesc> tiles;                        // gradient pass
    std::vector<std::vector<int64_t>> bucket_val;      // [output][k]: first tile value of size bucket k
    size_t n_tvals = 0;
    int64_t CH = 256;                                   // Phi pass: entries per chunk of the destination-major symmetric CSR
    std::vector<RowDesc> rows;
    std::vector<int64_t> out_chunk_begin;               // n_out + 1: first chunk of every output (its partials are contiguous)
    std::vector<int64_t> struct_entries, struct_slots;  // n_struct + 1: first entry / slot of every structure
    RawArray<int32_t> perm, cols;                       // entry -> slot, slot -> column (per structure)
    std::vector<int32_t> pslot;                         // regular rows (FoldReg)
    std::vector<uint16_t> rank_ab;
    std::vector<int32_t> invmap;                        // combine_grad
    int32_t *d_perm = nullptr;                          // device copy of perm (inside the arena)
    PlanLayout(int n_out, int nsym, int n_struct_)
        : n_struct(n_struct_), bucket_val(n_out), rows((size_t)n_out * nsym), out_chunk_begin(n_out + 1, 0),
          struct_entries(n_struct_ + 1, 0), struct_slots(n_struct_ + 1, 0) {}
};

// gradient pass: group-major tiles (descriptors only; values are scattered on the device), and the fused kernel's shape
static int layout_tiles(bluest_plan_t plan, PlanLayout &lay)
{
    const int n_out = (int)plan->outs.size();
    plan->kmax = 0;
    for (const auto &od : plan->outs) plan->kmax = std::max(plan->kmax, od.K);
    // tiles per workgroup of the fused kernel.  What bounds its tile stream is the rate at which ONE compute unit pulls bytes
    // that miss its L2 (~30 GB/s), so the tiles are spread over as many compute units as the device has (one workgroup of
    // 1024 threads fills a compute unit's registers): 184 workgroups of 15 tiles left 72 of 256 units idle at the headline size
    int tpb_max = 0;
    solve_grad_ku_dispatch(plan->kmax, [&](auto ku) { tpb_max = fused_tpb(pick_nt(plan->N), ku); });
    int64_t tiles_max = 1;
    for (const auto &od : plan->outs) {
        int64_t t = 0;
        for (int k = 1; k <= od.K; k++) t += (od.sizes[k - 1] + 63) / 64;
        tiles_max = std::max(tiles_max, t);
    }
    DeviceProps dp;
    HIP_TRY(device_props(plan->device, &dp));
    const int64_t wg_per_output = std::max<int64_t>(1, dp.cus / n_out);
    const int64_t tpb_cu = std::max<int64_t>(1, (tiles_max + wg_per_output - 1) / wg_per_output);
    plan->fused_tpb = (int)std::min<int64_t>(tpb_max, tpb_cu);
    std::vector<TileDesc> &tiles = lay.tiles;
    plan->grad_off.assign(n_out, 0);
    int64_t grad_len = 0;
    for (int o = 0; o < n_out; o++) {
        const OutputDesc &od = plan->outs[o];
        plan->grad_off[o] = grad_len;
        const size_t first_tile_of_output = tiles.size();
        lay.bucket_val[o].assign(od.K + 1, 0);
        int64_t li = 0;
        for (int k = 1; k <= od.K; k++) {
            const int64_t Lk = od.sizes[k - 1];
            lay.bucket_val[o][k] = (int64_t)lay.n_tvals;
            for (int64_t t0 = 0; t0 < Lk; t0 += 64) {
                TileDesc td;
                td.val_off = (int64_t)lay.n_tvals;
                td.grad_off = grad_len + li + t0;
                td.n_valid = (int32_t)std::min<int64_t>(64, Lk - t0);
                td.k = (int16_t)k; td.out = (int16_t)o;
                lay.n_tvals += (size_t)tile_slots(k) * 64;
                tiles.push_back(td);
            }
            li += Lk;
        }
        // first tile of the output is flagged; the list is padded to a multiple of FUSED_TPB tiles per output with empty
        // tiles so that a workgroup of the fused solve+gradient kernel never straddles two outputs
        if (tiles.size() > first_tile_of_output) tiles[first_tile_of_output].n_valid |= (1 << 30);
        while ((tiles.size() - first_tile_of_output) % plan->fused_tpb || tiles.size() == first_tile_of_output) {
            TileDesc td;
            td.val_off = 0; td.grad_off = 0; td.n_valid = (tiles.size() == first_tile_of_output) ? (1 << 30) : 0;
            td.k = 1; td.out = (int16_t)o;
            tiles.push_back(td);
        }
        const int bpo = (int)((tiles.size() - first_tile_of_output) / plan->fused_tpb);
        if (o == 0) plan->fused_bpo = bpo;
        else if (plan->fused_bpo != bpo) plan->fused_bpo = 0;
        grad_len += od.L_o;
    }
    lay.n_tvals = std::max<size_t>(lay.n_tvals, 128);       // the empty padding tiles read (and ignore) one slot pair at offset 0
    plan->grad_len = grad_len;
    plan->n_tiles = (int64_t)tiles.size();
    plan->spg_small = plan->L <= 4096 && plan->n_tiles <= 1024;
    return BLUEST_OK;
}

// Phi pass: destination-major symmetric CSR, positions only (counting sort of the entries by row, columns, row padding)
static int layout_phi(bluest_plan_t plan, PlanLayout &lay, PhaseTimer &timer)
{
    const int N = plan->N, n_out = (int)plan->outs.size(), nsym = plan->nsym, n_struct = lay.n_struct;
    int iters = 1;
    int64_t n_chunks = 0;
    std::vector<RowDesc> &rows = lay.rows;
    std::vector<int64_t> &out_chunk_begin = lay.out_chunk_begin, &struct_entries = lay.struct_entries, &struct_slots = lay.struct_slots;
    // parallel counting sort: slice s of S owns a contiguous range of the output's groups; it counts its entries per row,
    // the per-slice counts are prefix-summed into start offsets, then every slice writes the SLOT of its own entries -- rows
    // keep their entries in group order whatever S is, so the layout (and every summation order on the GPU) is independent
    // of threading
    std::vector<std::vector<int64_t>> counts(n_struct, std::vector<int64_t>(nsym, 0));
    int64_t max_row = 0;
    // slices per structure: as many as there are threads for them, but no slice below ~250 k (j, l) pairs -- spawning and joining
    // 16 threads costs more than counting the headline problem's 326 k pairs on one (the layout does not depend on S)
    int64_t pairs0 = 0;
    for (int k = 1; k <= plan->outs[0].K; k++) pairs0 += plan->outs[0].sizes[k - 1] * (int64_t)(k * (k + 1) / 2);
    const int S = (int)std::max<int64_t>(1, std::min<int64_t>(host_threads() / n_struct, pairs0 / 250000));
    std::vector<std::vector<int64_t>> slice_cnt((size_t)n_struct * S, std::vector<int64_t>(nsym, 0));
    auto for_groups_of_slice = [&](int o, int slice, auto &&body) {
        const OutputDesc &od = plan->outs[o];
        const int64_t lo = od.L_o * slice / S, hi = od.L_o * (slice + 1) / S;
        int64_t go = 0, eo = 0, l0 = 0;
        for (int k = 1; k <= od.K; k++) {
            const int64_t Lk = od.sizes[k - 1];
            const int ne = k * (k + 1) / 2;
            for (int64_t i = std::max<int64_t>(lo - l0, 0); i < std::min<int64_t>(hi - l0, Lk); i++)
                body(k, od.groups.data() + go + i * k, eo + i * ne, l0 + i);
            go += Lk * k; eo += Lk * ne; l0 += Lk;
        }
    };
    parallel_items(n_struct * S, [&](int item) {
        std::vector<int64_t> &cnt = slice_cnt[item];
        for_groups_of_slice(item / S, item % S, [&](int k, const int64_t *g, int64_t, int64_t) {
            for (int j = 0; j < k; j++)
                for (int l = j; l < k; l++) cnt[sym_row(N, (int)std::min(g[j], g[l]), (int)std::max(g[j], g[l]))]++;
        });
    });
    for (int o = 0; o < n_struct; o++)
        for (int r = 0; r < nsym; r++) {
            int64_t run = 0;
            for (int sl = 0; sl < S; sl++) { const int64_t c = slice_cnt[(size_t)o * S + sl][r]; slice_cnt[(size_t)o * S + sl][r] = run; run += c; }
            counts[o][r] = run;      // slice_cnt now holds each slice's start offset inside the row
            max_row = std::max(max_row, run);
        }
    timer.lap("count");
    while ((max_row + 256LL * iters - 1) / (256LL * iters) > 64 && iters < 1024) iters *= 2;
    const int64_t CH = lay.CH = 256LL * iters;
    plan->iters = iters;

    for (int o = 0; o < n_out; o++) {
        out_chunk_begin[o] = n_chunks;
        const std::vector<int64_t> &cnt = counts[plan->shared ? 0 : o];
        for (int a = 0; a < N; a++)
            for (int b = a; b < N; b++) {
                RowDesc &rd = rows[(size_t)o * nsym + sym_row(N, a, b)];
                const int64_t nc = (cnt[sym_row(N, a, b)] + CH - 1) / CH;
                rd.first_chunk = (int32_t)n_chunks;
                rd.n_chunks = (int32_t)nc;
                rd.out = (int16_t)o; rd.a = (int16_t)a; rd.b = (int16_t)b; rd.pad = 0;
                n_chunks += nc;
            }
    }
    out_chunk_begin[n_out] = n_chunks;
    if (n_chunks <= 0 || n_chunks * CH > 0x7fffffff0LL) return fail(BLUEST_ERR_ARG, "problem too large for one plan (%lld chunks)", (long long)n_chunks);
    plan->n_chunks = n_chunks;
    // slot of every packed-symmetric entry (reference order: group-major, upper triangle row by row) and the column
    // (= global index of the group) stored at that slot; per structure, relative to the structure's first chunk
    for (int o = 0; o < n_struct; o++) {
        int64_t ne_all = 0;
        for (int k = 1; k <= plan->outs[o].K; k++) ne_all += plan->outs[o].sizes[k - 1] * (k * (k + 1) / 2);
        struct_entries[o + 1] = struct_entries[o] + ne_all;
        struct_slots[o + 1] = struct_slots[o] + (out_chunk_begin[o + 1] - out_chunk_begin[o]) * CH;
    }
    if (struct_slots[n_struct] > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "problem too large for one plan (%lld slots per structure set)", (long long)struct_slots[n_struct]);
    lay.perm.reset((size_t)struct_entries[n_struct]);
    lay.cols.reset((size_t)struct_slots[n_struct]);
    parallel_items(n_struct * S, [&](int item) {
        const int o = item / S;
        std::vector<int64_t> &next = slice_cnt[item];     // start offsets, advanced as the slice writes
        const OutputDesc &od = plan->outs[o];
        const int64_t chunk0 = out_chunk_begin[o];
        int32_t *pm = lay.perm.data() + struct_entries[o];
        int32_t *cl = lay.cols.data() + struct_slots[o];
        for_groups_of_slice(o, item % S, [&](int k, const int64_t *g, int64_t e0, int64_t li) {
            int e = 0;
            for (int j = 0; j < k; j++)
                for (int l = j; l < k; l++, e++) {
                    const int rr = sym_row(N, (int)std::min(g[j], g[l]), (int)std::max(g[j], g[l]));
                    const int64_t pos = ((int64_t)rows[(size_t)o * nsym + rr].first_chunk - chunk0) * CH + next[rr]++;
                    pm[e0 + e] = (int32_t)pos;
                    cl[pos] = (int32_t)od.mapping[li];
                }
        });
    });
    // padding: value 0 (the device buffer is cleared), column = the row's first column (keeps max|m| per row exact, adds nothing)
    parallel_items(n_struct, [&](int o) {
        int32_t *cl = lay.cols.data() + struct_slots[o];
        for (int rr = 0; rr < nsym; rr++) {
            const RowDesc &rd = rows[(size_t)o * nsym + rr];
            const int64_t beg = ((int64_t)rd.first_chunk - out_chunk_begin[o]) * CH, end = beg + (int64_t)rd.n_chunks * CH;
            for (int64_t pos = beg + counts[o][rr]; pos < end; pos++) cl[pos] = cl[beg];
        }
    });
    return BLUEST_OK;
}

// regular rows (solve.hpp FoldReg): fixed partial strides per destination class when that wastes at most a quarter
static void layout_fold_reg(bluest_plan_t plan, PlanLayout &lay)
{
    const int N = plan->N, n_out = (int)plan->outs.size(), nsym = plan->nsym;
    const int64_t n_chunks = plan->n_chunks;
    plan->fold_reg = FoldReg{0, 0, nullptr};
    plan->slots_per_output = 0;
    int Cd = 0, Co = 0;
    for (const RowDesc &rd : lay.rows) { if (rd.a == rd.b) Cd = std::max<int>(Cd, rd.n_chunks); else Co = std::max<int>(Co, rd.n_chunks); }
    Co = std::max(Co, 1);
    const int64_t slots = (int64_t)N * Cd + (int64_t)(nsym - N) * Co;
    const bool no_reg = getenv("BLUEST_NO_REGULAR_FOLD") != nullptr;              // A/B switch, read per plan
    if (!no_reg && Cd >= 1 && Cd <= 32 && Co <= 32 && slots * n_out * 4 <= n_chunks * 5 && slots < 0x7fffffff / std::max(1, n_out)) {
        plan->fold_reg = FoldReg{Cd, Co, nullptr};
        for (int a = 0; a < N; a++) lay.rank_ab.push_back((uint16_t)(a | (a << 8)));
        for (int a = 0; a < N; a++) for (int b = a + 1; b < N; b++) lay.rank_ab.push_back((uint16_t)(a | (b << 8)));
        plan->slots_per_output = (int)slots;
        lay.pslot.assign((size_t)(plan->shared ? n_chunks / n_out : n_chunks), 0);
        std::vector<int> off_before(N + 1, 0);          // pairs a' < b' with a' < a
        for (int a = 0; a < N; a++) off_before[a + 1] = off_before[a] + (N - 1 - a);
        for (int o = 0; o < lay.n_struct; o++)
            for (int a = 0; a < N; a++)
                for (int b = a; b < N; b++) {
                    const RowDesc &rd = lay.rows[(size_t)o * nsym + sym_row(N, a, b)];
                    const int64_t first = (a == b) ? (int64_t)a * Cd : (int64_t)N * Cd + (int64_t)(off_before[a] + (b - a - 1)) * Co;
                    for (int j = 0; j < rd.n_chunks; j++)
                        lay.pslot[(size_t)(rd.first_chunk - (plan->shared ? lay.out_chunk_begin[o] : 0)) + j] = (int32_t)(first + (plan->shared ? 0 : (int64_t)o * slots) + j);
                }
    }
    plan->partial_stride = plan->fold_reg.Cd > 0 ? (int64_t)plan->slots_per_output * n_out : n_chunks;
}

// inverse maps for combine_grad
static void layout_invmap(bluest_plan_t plan, PlanLayout &lay)
{
    lay.invmap.assign(plan->outs.size() * plan->L, -1);
    parallel_items((int)plan->outs.size(), [&](int o) {
        for (int64_t li = 0; li < plan->outs[o].L_o; li++) lay.invmap[(size_t)o * plan->L + plan->outs[o].mapping[li]] = (int32_t)li;
    });
}

// the plan's device arena: reserve every array, clear what the scatter leaves unwritten, upload the host-built tables
static int arena_upload(bluest_plan_t plan, PlanLayout &lay)
{
    const int n_out = (int)plan->outs.size(), N = plan->N, max_candidates = plan->max_cand;
    const int64_t n_chunks = plan->n_chunks, CH = lay.CH;
    int rc;
    if (plan->d_scratch) { (void)pool_free(plan->d_scratch); plan->d_scratch = nullptr; plan->scratch_bytes = 0; }
    Arena arena;
    const size_t o_vals = arena.reserve((size_t)n_chunks * CH * sizeof(double)), o_cols = arena.reserve((size_t)n_chunks * CH * sizeof(int32_t));
    const size_t o_rows = arena.reserve(lay.rows.size() * sizeof(RowDesc));
    const size_t o_tiles = arena.reserve(lay.tiles.size() * sizeof(TileDesc)), o_tvals = arena.reserve(lay.n_tvals * sizeof(double));
    const size_t o_invmap = arena.reserve(lay.invmap.size() * sizeof(int32_t));
    const size_t o_goff = arena.reserve(plan->grad_off.size() * sizeof(int64_t));
    const size_t o_perm = arena.reserve(lay.perm.size() * sizeof(int32_t));
    const size_t o_partial = arena.reserve((size_t)max_candidates * plan->partial_stride * sizeof(double2));
    const size_t o_pslot = arena.reserve(lay.pslot.size() * sizeof(int32_t)), o_rankab = arena.reserve(lay.rank_ab.size() * sizeof(uint16_t));
    const size_t o_v = arena.reserve((size_t)max_candidates * n_out * N * sizeof(double));
    const size_t o_status = arena.reserve((size_t)max_candidates * n_out * sizeof(int32_t));
    const size_t o_ticket = arena.reserve(256);
    HIP_TRY(pool_alloc(&plan->d_arena, arena.bytes));
    arena.base = (char *)plan->d_arena;
    plan->d_vals = reinterpret_cast<double *>(arena.base + o_vals);
    plan->d_cols = reinterpret_cast<int32_t *>(arena.base + o_cols);
    plan->d_tvals = reinterpret_cast<double *>(arena.base + o_tvals);
    plan->d_partial = reinterpret_cast<double2 *>(arena.base + o_partial);
    plan->d_v = reinterpret_cast<double *>(arena.base + o_v);
    plan->d_status = reinterpret_cast<int32_t *>(arena.base + o_status);
    plan->d_ticket = reinterpret_cast<unsigned int *>(arena.base + o_ticket);
    // clear what the scatter kernels do not write (padding slots, padding lanes); then the small tables
    HIP_TRY(hipMemsetAsync(plan->d_vals, 0, (size_t)n_chunks * CH * sizeof(double), 0));
    HIP_TRY(hipMemsetAsync(plan->d_tvals, 0, lay.n_tvals * sizeof(double), 0));
    // columns: the structure's list sits at the structure's own chunk range (shared plans: output 0's range is the one the
    // Phi kernel reads; the other ranges stay unused)
    const std::vector<int64_t> &ocb = lay.out_chunk_begin, &ss = lay.struct_slots;
    if (plan->cols16) {
        RawArray<uint16_t> c16(lay.cols.size());
        for (size_t i = 0; i < lay.cols.size(); i++) c16.data()[i] = (uint16_t)lay.cols.data()[i];
        uint16_t *d16 = reinterpret_cast<uint16_t *>(plan->d_cols);
        for (int o = 0; o < lay.n_struct; o++)
            HIP_TRY(hipMemcpy(d16 + ocb[o] * CH, c16.data() + ss[o], (size_t)(ss[o + 1] - ss[o]) * sizeof(uint16_t), hipMemcpyHostToDevice));
    } else
    for (int o = 0; o < lay.n_struct; o++)
        HIP_TRY(hipMemcpy(plan->d_cols + ocb[o] * CH, lay.cols.data() + ss[o], (size_t)(ss[o + 1] - ss[o]) * sizeof(int32_t), hipMemcpyHostToDevice));
    if ((rc = upload(arena, o_rows, &plan->d_rows, lay.rows))) return rc;
    if ((rc = upload(arena, o_tiles, &plan->d_tiles, lay.tiles))) return rc;
    if ((rc = upload(arena, o_invmap, &plan->d_invmap, lay.invmap))) return rc;
    if ((rc = upload(arena, o_goff, &plan->d_goff, plan->grad_off))) return rc;
    if ((rc = upload(arena, o_perm, &lay.d_perm, lay.perm))) return rc;
    if ((rc = upload(arena, o_pslot, &plan->d_pslot, lay.pslot))) return rc;
    if (lay.pslot.empty()) plan->d_pslot = nullptr;
    uint16_t *d_rank_ab = nullptr;
    if ((rc = upload(arena, o_rankab, &d_rank_ab, lay.rank_ab))) return rc;
    plan->fold_reg.rank_ab = lay.rank_ab.empty() ? nullptr : d_rank_ab;
    return BLUEST_OK;
}

// scatter the values on the device (one launch per (output, group size) and layout); clear the partials and the ticket
static int scatter_values(bluest_plan_t plan, const PlanLayout &lay)
{
    for (int o = 0; o < (int)plan->outs.size(); o++) {
        const OutputDesc &od = plan->outs[o];
        const int st = plan->shared ? 0 : o;
        int64_t io = 0, go = 0, eo = 0;
        for (int k = 1; k <= od.K; k++) {
            const int64_t Lk = od.sizes[k - 1];
            const int ne = k * (k + 1) / 2;
            if (Lk > 0) {
                hipLaunchKernelGGL(k_fill_csr, dim3((unsigned)((Lk * ne + 255) / 256)), dim3(256), 0, 0, od.d_invcov + io, k, Lk,
                                   lay.d_perm + lay.struct_entries[st] + eo, plan->d_vals + lay.out_chunk_begin[o] * lay.CH);
                hipLaunchKernelGGL(k_fill_tiles, dim3((unsigned)((Lk * (ne + k) + 255) / 256)), dim3(256), 0, 0, od.d_invcov + io,
                                   od.d_groups + go, k, Lk, plan->d_tvals + lay.bucket_val[o][k]);
            }
            io += Lk * k * k; go += Lk * k; eo += Lk * ne;
        }
    }
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(0));
    // regular rows read slots no chunk writes: they stay zero for the plan's life
    if (plan->fold_reg.Cd > 0) {
        HIP_TRY(hipMemsetAsync(plan->d_partial, 0, (size_t)plan->max_cand * plan->partial_stride * sizeof(double2), 0));
        HIP_TRY(hipStreamSynchronize(0));
    }
    HIP_TRY(hipMemset(plan->d_ticket, 0, 256));
    return BLUEST_OK;
}

extern "C" int bluest_plan_finalize(bluest_plan_t plan, int max_candidates)
{
    if (!plan) return fail(BLUEST_ERR_ARG, "plan is NULL");
    if (plan->finalized) return fail(BLUEST_ERR_STATE, "plan already finalized");
    if (plan->outs.empty()) return fail(BLUEST_ERR_STATE, "plan has no outputs");
    if (max_candidates <= 0 || max_candidates > 65535) return fail(BLUEST_ERR_ARG, "max_candidates=%d out of range", max_candidates);
    const int N = plan->N, n_out = (int)plan->outs.size();
    PhaseTimer timer("plan_finalize");

    plan->nsym = N * (N + 1) / 2;
    if (N > 64 || plan->nsym > 2080) return fail(BLUEST_ERR_ARG, "N=%d: the fused kernel's argument word holds N <= 64, nsym <= 2080", N);
    plan->max_cand = max_candidates;
    plan->shared = true;
    for (int o = 1; o < n_out; o++) {
        const OutputDesc &x = plan->outs[0], &y = plan->outs[o];
        if (x.K != y.K || x.sizes != y.sizes || x.groups != y.groups || x.mapping != y.mapping) { plan->shared = false; break; }
    }
    // distinct STRUCTURES: with identical group lists and mappings every output has the same rows, chunks and slots, so the
    // counting sort runs once and the other outputs reuse its result shifted by their chunk base
    PlanLayout lay(n_out, plan->nsym, plan->shared ? 1 : n_out);
    int rc;
    if ((rc = layout_tiles(plan, lay))) return rc;
    plan->identity = plan->shared && plan->outs[0].L_o == plan->L;
    for (int64_t li = 0; plan->identity && li < plan->L; li++) plan->identity = plan->outs[0].mapping[li] == li;
    if ((rc = layout_phi(plan, lay, timer))) return rc;
    layout_fold_reg(plan, lay);
    timer.lap("CSR slots + columns");
    layout_invmap(plan, lay);
    plan->cols16 = plan->L <= 65536 && getenv("BLUEST_COLS32") == nullptr;       // (A/B switch: BLUEST_COLS32=1 keeps int32 columns)
    plan->phi_ob_forced = 0;                                                      // (A/B switch: BLUEST_PHI_OB=2|4|8, see phi_ob)
    if (const char *e = getenv("BLUEST_PHI_OB")) { const int v = atoi(e); if (v == 2 || v == 4 || v == 8) plan->phi_ob_forced = v; }
    plan->phi_bytes = plan->n_chunks * lay.CH * 8 + (plan->shared ? plan->n_chunks / n_out : plan->n_chunks) * lay.CH * (plan->cols16 ? 2 : 4) + plan->n_chunks * 16;
    plan->grad_bytes = (int64_t)lay.n_tvals * 8 + plan->grad_len * 8;
    const char *nt_env = getenv("BLUEST_TILE_NT");              // A/B switch, read per plan: 0 = plain loads
    plan->tile_nt = nt_env ? atoi(nt_env) != 0 : true;
    timer.lap("tile descriptors + inverse maps");
    if ((rc = arena_upload(plan, lay))) return rc;
    timer.lap("device arena + small uploads");
    if ((rc = scatter_values(plan, lay))) return rc;
    plan->finalized = true;
    if ((rc = mf_finalize(plan))) return rc;      // matrix-free evaluation for plans that qualify (matfree.hip)

    timer.lap("device scatter of the values");
    return BLUEST_OK;
}

int plan_ready(bluest_plan_t plan, int n_cand)
{
    if (!plan) return fail(BLUEST_ERR_ARG, "plan is NULL");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    if (n_cand <= 0 || n_cand > plan->max_cand) return fail(BLUEST_ERR_ARG, "n_cand=%d outside 1..%d", n_cand, plan->max_cand);
    return BLUEST_OK;
}

extern "C" int bluest_plan_output_layout(bluest_plan_t plan, int output, int *K, int64_t *sizes, int64_t *mapping)
{
    if (!plan || !K) return fail(BLUEST_ERR_ARG, "null pointer");
    if (output < 0 || output >= (int)plan->outs.size()) return fail(BLUEST_ERR_ARG, "output %d out of range", output);
    const OutputDesc &od = plan->outs[output];
    *K = od.K;
    if (sizes) std::copy(od.sizes.begin(), od.sizes.end(), sizes);
    if (mapping) std::copy(od.mapping.begin(), od.mapping.end(), mapping);
    return BLUEST_OK;
}

// The working set of the solver: a plan over a sub-list of the parent's groups, built natively -- group lists and mappings are
// filtered on the host (they live there), the k x k pseudo-inverse blocks are gathered device to device.
extern "C" int bluest_plan_restrict(bluest_plan_t parent, const int64_t *keep, int64_t n_keep, int max_candidates, bluest_plan_t *restricted)
{
    if (!parent || !keep || !restricted) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!parent->finalized) return fail(BLUEST_ERR_STATE, "parent plan not finalized");
    if (n_keep <= 0 || n_keep > parent->L) return fail(BLUEST_ERR_ARG, "n_keep=%lld out of range", (long long)n_keep);
    PhaseTimer timer("plan_restrict");
    DeviceScope scope(parent->device);                   // the sub-plan lives where its parent's inverses are
    std::vector<int32_t> pos((size_t)parent->L, -1);
    for (int64_t i = 0; i < n_keep; i++) {
        if (keep[i] < 0 || keep[i] >= parent->L || (i > 0 && keep[i] <= keep[i - 1]))
            return fail(BLUEST_ERR_ARG, "keep must be strictly ascending indices in [0, L_global)");
        pos[(size_t)keep[i]] = (int32_t)i;
    }
    bluest_plan_t sub = nullptr;
    int rc = bluest_plan_create(&sub, parent->N, n_keep);
    if (rc) return rc;
    const int n_out = (int)parent->outs.size();
    // selection per output (host), and ONE upload of all gather descriptors
    std::vector<int64_t> src, dst;
    std::vector<int32_t> kk;
    std::vector<int64_t> first_of_output(n_out + 1, 0);
    std::vector<OutputDesc> nods((size_t)n_out);
    for (int o = 0; o < n_out; o++) {
        const OutputDesc &od = parent->outs[o];
        OutputDesc &nd = nods[o];
        nd.K = od.K;
        nd.sizes.assign(od.K, 0);
        bool has0 = false;
        int64_t t0 = 0, goff = 0, ioff = 0, dtot = 0;
        for (int k = 1; k <= od.K; k++) {
            const int64_t Lk = od.sizes[k - 1];
            for (int64_t t = 0; t < Lk; t++) {
                const int32_t q = pos[(size_t)od.mapping[t0 + t]];
                if (q < 0) continue;
                const int64_t *gp = od.groups.data() + goff + t * k;
                for (int j = 0; j < k; j++) has0 = has0 || gp[j] == 0;
                nd.groups.insert(nd.groups.end(), gp, gp + k);
                nd.mapping.push_back(q);
                nd.sizes[k - 1]++;
                src.push_back(ioff + t * k * k);
                dst.push_back(dtot);
                kk.push_back(k);
                dtot += (int64_t)k * k;
            }
            t0 += Lk; goff += Lk * k; ioff += Lk * k * k;
        }
        nd.L_o = (int64_t)nd.mapping.size();
        first_of_output[o + 1] = (int64_t)src.size();
        if (nd.L_o == 0 || !has0) {
            bluest_plan_destroy(sub);
            return fail(BLUEST_ERR_ARG, "restricted plan: output %d would not sample model 0", o);
        }
    }
    timer.lap("select groups");
    const int64_t n_all = (int64_t)src.size();
    void *d = nullptr;
    const size_t b64 = (size_t)n_all * sizeof(int64_t), b32 = ((size_t)n_all * sizeof(int32_t) + 7) / 8 * 8;
    hipError_t e = pool_alloc(&d, 2 * b64 + b32);
    if (e != hipSuccess) { bluest_plan_destroy(sub); HIP_TRY(e); }
    int64_t *d_src = (int64_t *)d, *d_dst = d_src + n_all;
    int32_t *d_k = (int32_t *)(d_dst + n_all);
    e = hipMemcpy(d_src, src.data(), b64, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_dst, dst.data(), b64, hipMemcpyHostToDevice);
    if (e == hipSuccess) e = hipMemcpy(d_k, kk.data(), (size_t)n_all * sizeof(int32_t), hipMemcpyHostToDevice);
    for (int o = 0; o < n_out && e == hipSuccess; o++) {
        OutputDesc &nd = nods[o];
        if (output_to_device(sub, nd) != BLUEST_OK) { output_release(nd); e = hipErrorOutOfMemory; break; }
        const int64_t f = first_of_output[o], n = first_of_output[o + 1] - f;
        hipLaunchKernelGGL(k_gather_blocks, dim3((unsigned)n), dim3(64), 0, 0, parent->outs[o].d_invcov, d_src + f, d_dst + f, d_k + f, n,
                           nd.d_invcov);
        sub->outs.push_back(std::move(nd));
    }
    if (e == hipSuccess) e = hipDeviceSynchronize();     // the descriptors are released below
    (void)pool_free(d, e == hipSuccess);                 // after a HIP error the block goes back to the runtime, not to the cache
    if (e != hipSuccess) { bluest_plan_destroy(sub); HIP_TRY(e); }
    timer.lap("gather inverses (device)");
    rc = bluest_plan_finalize(sub, max_candidates);
    if (rc) { bluest_plan_destroy(sub); return rc; }
    *restricted = sub;
    return BLUEST_OK;
}

extern "C" int bluest_plan_n_outputs(bluest_plan_t plan, int *n)
{
    if (!plan || !n) return fail(BLUEST_ERR_ARG, "null pointer");
    *n = (int)plan->outs.size();
    return BLUEST_OK;
}

extern "C" int bluest_plan_grad_layout(bluest_plan_t plan, int64_t *grad_len, int64_t *offsets)
{
    if (!plan) return fail(BLUEST_ERR_ARG, "plan is NULL");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    if (grad_len) *grad_len = plan->grad_len;
    if (offsets) for (size_t o = 0; o < plan->outs.size(); o++) offsets[o] = plan->grad_off[o];
    return BLUEST_OK;
}

extern "C" int bluest_plan_traffic(bluest_plan_t plan, int64_t *phi_bytes, int64_t *grad_bytes)
{
    if (!plan) return fail(BLUEST_ERR_ARG, "plan is NULL");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    if (phi_bytes) *phi_bytes = plan->phi_bytes;
    if (grad_bytes) *grad_bytes = plan->grad_bytes;
    return BLUEST_OK;
}

extern "C" int bluest_plan_phi_len(bluest_plan_t plan, int64_t *len)
{
    if (!plan || !len) return fail(BLUEST_ERR_ARG, "null pointer");
    *len = (int64_t)plan->outs.size() * (plan->N * plan->N + 2 * plan->N + 1);
    return BLUEST_OK;
}

static void launch_grad(bluest_plan_t plan, const double *v_dev, const int32_t *status_dev, int n_cand, double *grad_dev,
                        int64_t grad_stride, hipStream_t st)
{
    GradTilesKuSet::dispatch(plan->kmax, [&](auto ku) {
        hipLaunchKernelGGL((k_grad_tiles<decltype(ku)::value>), dim3((unsigned)((plan->n_tiles + 3) / 4)), dim3(256), 0, st, plan->d_tiles,
                           plan->n_tiles, plan->d_tvals, v_dev, status_dev, plan->N, (int)plan->outs.size(), n_cand, grad_dev, grad_stride, plan->gate);
    });
}

// the solve from Phi records (n_cand candidates): var / v / status
static void launch_solve_from_record(bluest_plan_t plan, const double *rec, int n_cand, double delta, int want_v, double *var_dev,
                                     double *v_dev, int32_t *status_dev, hipStream_t st)
{
    const int n_out = (int)plan->outs.size();
    nt_dispatch(plan->N, [&](auto nt) {
        hipLaunchKernelGGL((k_solve_from_record<decltype(nt)::value>), dim3(n_out, n_cand), dim3(64), 0, st, plan->N, n_out, rec, delta, want_v,
                           var_dev, v_dev, status_dev);
    });
}

// the fused solve + gradient pass of one candidate: from a Phi record (rec != NULL, sharded plans) or from the chunk partials the Phi
// pass left; optionally the SPG line-search decision in the tail (dec_state) or the multiplicative update instead of the gradient (ma)
static void launch_solve_grad(bluest_plan_t plan, const double *rec, double delta, double *var_dev, int32_t *status_dev, double *grad_dev,
                              double *dec_state, int dec_last, int32_t *dec_enable, MaTail ma, hipStream_t st)
{
    const int n_out = (int)plan->outs.size();
    // (bpo, n_out) when every output has bpo workgroups -- the kernel reads its output off the grid --, else one row of workgroups
    const dim3 grid = plan->fused_bpo > 0 ? dim3((unsigned)plan->fused_bpo, (unsigned)n_out) : dim3((unsigned)(plan->n_tiles / plan->fused_tpb));
    const uint32_t flags = (rec ? SG_HAS_REC : 0u) | (plan->gate ? SG_HAS_GATE : 0u) | (dec_state ? SG_HAS_SPG : 0u);
    nt_dispatch(plan->N, [&](auto nt) { solve_grad_ku_dispatch(plan->kmax, [&](auto ku) {
        constexpr int NT = decltype(nt)::value, KU = decltype(ku)::value;
        hipLaunchKernelGGL((k_solve_grad<NT, KU>), grid, dim3(64 * (fused_tpb(NT, KU) + 1)), 0, st, plan->d_partial, plan->fold_reg.rank_ab, plan->d_rows,
                           plan->d_tiles, (uint32_t)plan->N | (uint32_t)plan->nsym << 8, plan->fold_reg.Cd, plan->fold_reg.Co, plan->fused_bpo, flags,
                           n_out, plan->fused_tpb, (int)plan->tile_nt, rec, delta, plan->d_tvals, var_dev, plan->d_v, status_dev, grad_dev,
                           plan->gate, dec_state, dec_last, dec_enable, plan->d_ticket, ma);
    }); });
}

// outputs per wavefront of the shared Phi pass (k_phi_chunks_shared<OB>) for a launch of n_cand candidates, 0: the plain
// k_phi_chunks.  A wider OB reads the column stream and gathers m once for more outputs and spends fewer instructions per output
// (profiles/r07_isa_counts.txt), but leaves fewer wavefronts to hide the latency of the stream behind.
// One candidate: the widest OB of PhiObSet that keeps PHI_MIN_WAVES wavefronts, else the narrowest.  The 2304 (nine wavefronts per
// compute unit) rests on ONE shape: at the headline size (1160 chunks per output, 8 outputs) OB = 4 with 2320 wavefronts takes
// 3.3-3.4 us against 4.1-4.2 us of OB = 2 with 4640 (profiles/r07_step_parts_ab.txt), and nothing was measured between 2080
// wavefronts -- where the plans of tests/test_gpu_launch_matrix.py keep the narrower OB -- and 2320.  (The 4096 that stood here before
// was measured in round 3 with six ds_bpermute trips per sum in the tail: OB = 8 6.9 us, 4 5.5 us, 2 5.1 us, 1 6.1 us.)
// A batch (n_cand > 1) takes the same OB: every wavefront loops over the candidates, and the m gathers that bound the pass are
// repeated per block of outputs, so a wider OB pays more there (n_cand = 16 at the headline size: 28 us at OB = 4 against 42 us at
// OB = 2), but the widest is not the best one -- OB = 8 with 1160 wavefronts takes 32 us (profiles/r07_batch_ob.txt).
// BLUEST_PHI_OB (read per plan at finalize) forces an OB for shared plans of two or more outputs: an A/B switch.
static const int64_t PHI_MIN_WAVES = 2304;
static int phi_ob(const bluest_plan_s *p, int n_cand)
{
    (void)n_cand;      // one rule for every n_cand, see above; launch_chunks and bluest_plan_launch_config both ask here
    const int n_out = (int)p->outs.size();
    if (!p->shared || n_out < 2) return 0;
    if (p->phi_ob_forced) return p->phi_ob_forced;
    const int64_t ncpo = p->n_chunks / n_out;
    for (int i = PhiObSet::count - 1; i > 0; i--) {
        const int ob = PhiObSet::values[i];
        if (ob <= n_out && ncpo * ((n_out + ob - 1) / ob) >= PHI_MIN_WAVES) return ob;
    }
    return PhiObSet::values[0];
}

static void launch_chunks(bluest_plan_t p, const double *m, int n_cand, int64_t m_stride, hipStream_t st)
{
    const int n_out = (int)p->outs.size();
    // what the kernels' entry takes as it is: the entries of a chunk, and the top-bit flags next to n_out
    const uint32_t CH = (uint32_t)p->iters * 256u;
    const uint32_t n_out_flags = (uint32_t)n_out | (p->gate ? PHI_HAS_GATE : 0u);
    // one wavefront per workgroup of the chunk kernels (WPB = 1): single-wavefront workgroups drain earliest at the kernel's end
    // (same-box A/B at the headline size, two runs each: step 12.86 / 12.26 / 12.05 us with 4 / 2 / 1 wavefronts, 13.8 with 16)
    if (const int ob = phi_ob(p, n_cand)) {
        const int64_t ncpo = p->n_chunks / n_out;
        PhiObSet::dispatch(ob, [&](auto obc) {
            constexpr int OB = decltype(obc)::value;
#define LCS2(COLT) hipLaunchKernelGGL((k_phi_chunks_shared<OB, 1, COLT>), dim3((unsigned)ncpo, (n_out + OB - 1) / OB), dim3(64), 0, st, \
                                   p->d_vals, reinterpret_cast<const COLT *>(p->d_cols), m, p->d_pslot, CH, (uint32_t)ncpo, (uint64_t)ncpo * CH * sizeof(double), n_out_flags, n_cand, \
                                   p->gate, m_stride, p->partial_stride, p->slots_per_output, p->d_partial)
            if (p->cols16) LCS2(uint16_t); else LCS2(int32_t);
#undef LCS2
        });
        return;
    }
#define LPC(COLT) hipLaunchKernelGGL((k_phi_chunks<1, COLT>), dim3((unsigned)p->n_chunks), dim3(64), 0, st, p->d_vals, \
                                  reinterpret_cast<const COLT *>(p->d_cols), m, p->d_pslot, CH, (uint32_t)p->n_chunks, (uint64_t)0, n_out_flags, n_cand, \
                                  p->gate, m_stride, p->partial_stride, p->slots_per_output, p->d_partial)
    if (p->cols16) LPC(uint16_t); else LPC(int32_t);
#undef LPC
}

extern "C" int bluest_plan_phi_chunks(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, void *stream)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!m_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (n_cand > 1 && m_stride < plan->L) return fail(BLUEST_ERR_ARG, "m_stride < L_global");
    launch_chunks(plan, m_dev, n_cand, m_stride, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

extern "C" int bluest_plan_phi(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, double *phi_dev, void *stream)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!m_dev || !phi_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (n_cand > 1 && m_stride < plan->L) return fail(BLUEST_ERR_ARG, "m_stride < L_global");
    hipStream_t st = (hipStream_t)stream;
    const int n_out = (int)plan->outs.size();
    if (plan->matfree && n_cand == 1 && !plan->gate) return mf_phi_record(plan, m_dev, phi_dev, nullptr, st);
    launch_chunks(plan, m_dev, n_cand, m_stride, st);
    nt_dispatch(plan->N, [&](auto nt) {
        hipLaunchKernelGGL((k_fold_to_record<decltype(nt)::value>), dim3(n_out, n_cand), dim3(fold_threads(nt)), 0, st, plan->N, n_out, plan->d_rows,
                           plan->nsym, plan->fold_reg, plan->d_partial, plan->partial_stride, phi_dev);
    });
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

extern "C" int bluest_plan_solve(bluest_plan_t plan, const double *phi_dev, int n_cand, double delta, double *var_dev,
                                 double *v_dev, int32_t *status_dev, void *stream)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!phi_dev || !var_dev || !v_dev || !status_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    launch_solve_from_record(plan, phi_dev, n_cand, delta, 1, var_dev, v_dev, status_dev, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

extern "C" int bluest_plan_solve_pinv(bluest_plan_t plan, const double *phi_dev, int n_cand, double delta, double *var_dev,
                                      double *v_dev, int32_t *status_dev, void *stream)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!phi_dev || !var_dev || !v_dev || !status_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    const int n_out = (int)plan->outs.size(), N = plan->N;
    const size_t lds = (size_t)2 * N * (N + 1) * sizeof(double);      // 66 560 bytes at N = 64
    // dynamic LDS beyond the default needs the attribute (per device, as for k_phi_matfree in matfree.hip)
    if (lds > (48u << 10)) (void)hipFuncSetAttribute((const void *)k_pinv_from_record, hipFuncAttributeMaxDynamicSharedMemorySize, (int)lds);
    hipLaunchKernelGGL(k_pinv_from_record, dim3(n_out, n_cand), dim3(64), lds, (hipStream_t)stream, N, n_out, phi_dev, delta, var_dev,
                       v_dev, status_dev);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

extern "C" int bluest_plan_grad(bluest_plan_t plan, const double *v_dev, const int32_t *status_dev, int n_cand,
                                double *grad_dev, int64_t grad_stride, void *stream)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!v_dev || !status_dev || !grad_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (n_cand > 1 && grad_stride < plan->grad_len) return fail(BLUEST_ERR_ARG, "grad_stride < grad_len");
    if (plan->mf_gradient && n_cand == 1 && !plan->gate) return mf_grad(plan, v_dev, status_dev, grad_dev, (hipStream_t)stream);
    launch_grad(plan, v_dev, status_dev, n_cand, grad_dev, grad_stride, (hipStream_t)stream);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

static int plan_eval(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, double delta,
                     double *var_dev, double *grad_dev, int64_t grad_stride, int32_t *status_dev, void *stream,
                     double *dec_state, int dec_last, int32_t *dec_enable, MaTail ma = MaTail{nullptr, nullptr, nullptr, nullptr});

extern "C" int bluest_plan_eval(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, double delta,
                                double *var_dev, double *grad_dev, int64_t grad_stride, int32_t *status_dev, void *stream)
{
    return plan_eval(plan, m_dev, n_cand, m_stride, delta, var_dev, grad_dev, grad_stride, status_dev, stream, nullptr, 0, nullptr);
}

// group-sharded plans: the second half of an evaluation FROM the all-reduced Phi record in one launch -- redundant solve in
// every workgroup, gradient tiles of this GPU's shard, optionally the SPG line-search decision in the tail
extern "C" int bluest_plan_solve_grad(bluest_plan_t plan, const double *rec_dev, double delta, double *var_dev, double *grad_dev,
                                      int32_t *status_dev, double *state_dev, int last_slot, int32_t *enable_dev, void *stream)
{
    int rc = plan_ready(plan, 1); if (rc) return rc;
    if (!rec_dev || !var_dev || !grad_dev || !status_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (state_dev && !enable_dev) return fail(BLUEST_ERR_ARG, "the decision needs enable_dev");
    const int n_out = (int)plan->outs.size();
    if (state_dev && n_out > SPG_MAX_OUT) return fail(BLUEST_ERR_ARG, "more than %d outputs", SPG_MAX_OUT);
    hipStream_t st = (hipStream_t)stream;
    if (plan->mf_gradient && !state_dev && !plan->gate) return mf_solve_grad(plan, rec_dev, delta, var_dev, status_dev, grad_dev, st);
    launch_solve_grad(plan, rec_dev, delta, var_dev, status_dev, grad_dev, state_dev, last_slot, enable_dev, MaTail{nullptr, nullptr, nullptr, nullptr}, st);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

extern "C" int bluest_plan_eval_decide(bluest_plan_t plan, const double *m_dev, double delta, double *var_dev, int32_t *status_dev,
                                       double *state_dev, int last_slot, int32_t *enable_dev, void *stream)
{
    if (!state_dev || !enable_dev || !status_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (plan && (int)plan->outs.size() > SPG_MAX_OUT) return fail(BLUEST_ERR_ARG, "more than %d outputs", SPG_MAX_OUT);
    return plan_eval(plan, m_dev, 1, 0, delta, var_dev, nullptr, 0, status_dev, stream, state_dev, last_slot, enable_dev);
}

extern "C" int bluest_plan_eval_grad_decide(bluest_plan_t plan, const double *m_dev, double delta, double *var_dev, double *grad_dev,
                                            int32_t *status_dev, double *state_dev, int last_slot, int32_t *enable_dev, void *stream)
{
    if (!state_dev || !enable_dev || !status_dev || !grad_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (plan && (int)plan->outs.size() > SPG_MAX_OUT) return fail(BLUEST_ERR_ARG, "more than %d outputs", SPG_MAX_OUT);
    return plan_eval(plan, m_dev, 1, 0, delta, var_dev, grad_dev, plan ? plan->grad_len : 0, status_dev, stream, state_dev, last_slot, enable_dev);
}

static int plan_eval(bluest_plan_t plan, const double *m_dev, int n_cand, int64_t m_stride, double delta,
                     double *var_dev, double *grad_dev, int64_t grad_stride, int32_t *status_dev, void *stream,
                     double *dec_state, int dec_last, int32_t *dec_enable, MaTail ma)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!m_dev || !var_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (n_cand > 1 && m_stride < plan->L) return fail(BLUEST_ERR_ARG, "m_stride < L_global");
    if (grad_dev && n_cand > 1 && grad_stride < plan->grad_len) return fail(BLUEST_ERR_ARG, "grad_stride < grad_len");
    hipStream_t st = (hipStream_t)stream;
    const int n_out = (int)plan->outs.size();
    int32_t *status = status_dev ? status_dev : plan->d_status;
    if (plan->matfree && n_cand == 1 && !dec_state && !plan->gate) {
        // matrix-free: Phi pass -> record -> (solve + gradient | solve) -- no stored inverse is read
        const double *rec = nullptr;
        if ((rc = mf_phi_record(plan, m_dev, nullptr, &rec, st))) return rc;
        if (grad_dev) return mf_solve_grad(plan, rec, delta, var_dev, status, grad_dev, st, ma);
        launch_solve_from_record(plan, rec, 1, delta, plan->always_v ? 1 : 0, var_dev, plan->d_v, status, st);
        HIP_TRY(hipGetLastError());
        return BLUEST_OK;
    }
    launch_chunks(plan, m_dev, n_cand, m_stride, st);
    if (plan->mf_gradient && grad_dev && n_cand == 1 && !dec_state && !plan->gate)
        return mf_solve_grad(plan, nullptr, delta, var_dev, status, grad_dev, st, ma);  // stored Phi pass + fold, solve and matrix-free gradient
    // fused solve + gradient pass (2 launches per evaluation); groups larger than 12 take the generic tile code inside it
    if (grad_dev && n_cand == 1) {
        launch_solve_grad(plan, nullptr, delta, var_dev, status, grad_dev, dec_state, dec_last, dec_enable, ma, st);
        HIP_TRY(hipGetLastError());
        return BLUEST_OK;
    }
    const int want = (grad_dev || plan->always_v) ? 1 : 0;
    nt_dispatch(plan->N, [&](auto nt) {
        hipLaunchKernelGGL((k_solve_from_chunks<decltype(nt)::value>), dim3(n_out, n_cand), dim3(fold_threads(nt)), 0, st, plan->N, n_out, plan->d_rows,
                           plan->nsym, plan->fold_reg, plan->d_partial, plan->partial_stride, delta, want, var_dev, plan->d_v, status, plan->gate,
                           dec_state, dec_last, dec_enable, plan->d_ticket);
    });
    if (grad_dev)
        launch_grad(plan, plan->d_v, status, n_cand, grad_dev, grad_stride, st);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

extern "C" int bluest_plan_is_identity(bluest_plan_t plan, int *yes)
{
    if (!plan || !yes) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    *yes = plan->identity ? 1 : 0;
    return BLUEST_OK;
}

// widest group the multiplicative tail of the fused solve + gradient kernel handles (its unrolled tile paths), 0: plan does not qualify
static int eval_ma_kmax(const bluest_plan_s *plan)
{
    if (plan->outs.size() != 1 || !plan->identity || plan->gate) return 0;
    return plan->matfree ? 8 : 12;
}

extern "C" int bluest_plan_eval_ma_kmax(bluest_plan_t plan, int *kmax)
{
    if (!plan || !kmax) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    *kmax = eval_ma_kmax(plan);
    return BLUEST_OK;
}

extern "C" int bluest_plan_kmax(bluest_plan_t plan, int *kmax)
{
    if (!plan || !kmax) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    *kmax = plan->kmax;
    return BLUEST_OK;
}

// the instantiation every kernel family of an evaluation takes on this plan, from the helpers the launchers call (phi_ob, the
// InstSet dispatchers, fused_tpb, fold_threads, mf_instantiation)
extern "C" int bluest_plan_launch_config(bluest_plan_t plan, int n_cand, int32_t *cfg)
{
    if (!plan || !cfg) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    if (n_cand <= 0 || n_cand > plan->max_cand) return fail(BLUEST_ERR_ARG, "n_cand=%d outside 1..%d", n_cand, plan->max_cand);
    std::fill(cfg, cfg + BLUEST_LC_COUNT, 0);
    const bool one = n_cand == 1 && !plan->gate;
    cfg[BLUEST_LC_PATH] = (one && plan->matfree) ? 2 : (one && plan->mf_gradient) ? 3 : (n_cand == 1) ? 1 : 0;
    cfg[BLUEST_LC_PHI_OB] = phi_ob(plan, n_cand);
    cfg[BLUEST_LC_COLS16] = plan->cols16 ? 1 : 0;
    nt_dispatch(plan->N, [&](auto nt) {
        cfg[BLUEST_LC_NT] = decltype(nt)::value;
        cfg[BLUEST_LC_FOLD_THREADS] = fold_threads(decltype(nt)::value);
        solve_grad_ku_dispatch(plan->kmax, [&](auto ku) {
            cfg[BLUEST_LC_SOLVE_GRAD_KU] = decltype(ku)::value;
            cfg[BLUEST_LC_FUSED_TPB] = fused_tpb(decltype(nt)::value, decltype(ku)::value);
        });
    });
    cfg[BLUEST_LC_TILES_PER_WG] = plan->fused_tpb;
    GradTilesKuSet::dispatch(plan->kmax, [&](auto ku) { cfg[BLUEST_LC_GRAD_TILES_KU] = decltype(ku)::value; });
    cfg[BLUEST_LC_MATFREE] = plan->matfree ? 1 : (plan->mf_gradient ? 2 : 0);
    if (plan->mf_gradient) mf_instantiation(plan, &cfg[BLUEST_LC_MF_NW], &cfg[BLUEST_LC_MF_NT], &cfg[BLUEST_LC_MF_KU]);
    cfg[BLUEST_LC_ITERS] = plan->iters;
    cfg[BLUEST_LC_KMAX] = plan->kmax;
    return BLUEST_OK;
}

extern "C" int bluest_launch_set(int axis, int32_t *values, int cap, int *n)
{
    if (!n || (cap > 0 && !values)) return fail(BLUEST_ERR_ARG, "null pointer");
    std::vector<int32_t> s;
    auto add = [&](int v) { if (std::find(s.begin(), s.end(), v) == s.end()) s.push_back(v); };
    switch (axis) {
    case BLUEST_LC_PHI_OB: for (int v : PhiObSet::values) add(v); break;
    case BLUEST_LC_NT: for (int v : NtSet::values) add(v); break;
    case BLUEST_LC_FOLD_THREADS: for (int v : NtSet::values) add(fold_threads(v)); break;
    case BLUEST_LC_SOLVE_GRAD_KU: for (int v : SolveGradKuSet::values) add(v); break;
    case BLUEST_LC_FUSED_TPB: for (int nt : NtSet::values) for (int ku : SolveGradKuSet::values) add(fused_tpb(nt, ku)); break;
    case BLUEST_LC_GRAD_TILES_KU: for (int v : GradTilesKuSet::values) add(v); break;
    case BLUEST_LC_MF_NW: case BLUEST_LC_MF_NT: case BLUEST_LC_MF_KU: mf_instantiation_set(axis, s); break;
    default: return fail(BLUEST_ERR_ARG, "axis %d has no instantiation set", axis);
    }
    *n = (int)s.size();
    for (int i = 0; i < (int)s.size() && i < cap; i++) values[i] = s[(size_t)i];
    return BLUEST_OK;
}

// phase 1 of the second-order finish on a single-output plan: one evaluation of m_dev whose fused solve + gradient kernel applies the
// multiplicative update to x_dev / m_dev itself (no gradient array, no third launch); var / status as bluest_plan_eval leaves them
extern "C" int bluest_plan_eval_ma(bluest_plan_t plan, double *m_dev, double *var_dev, int32_t *status_dev, const double *s_dev,
                                   const double *cc_dev, double *x_dev, void *stream)
{
    if (!plan || !m_dev || !var_dev || !status_dev || !s_dev || !cc_dev || !x_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (!plan->finalized) return fail(BLUEST_ERR_STATE, "plan not finalized");
    if (plan->outs.size() != 1 || !plan->identity || plan->gate || plan->kmax > eval_ma_kmax(plan))
        return fail(BLUEST_ERR_STATE, "bluest_plan_eval_ma: one output on all groups under the identity mapping only, groups of at most %d models",
                    eval_ma_kmax(plan));
    // (the gradient pointer only selects the fused kernel: with the tail on, nothing is written through it)
    return plan_eval(plan, m_dev, 1, 0, 0.0, var_dev, plan->d_v, plan->grad_len, status_dev, stream, nullptr, 0, nullptr, MaTail{x_dev, cc_dev, m_dev, s_dev});
}

extern "C" int bluest_plan_combine_grad(bluest_plan_t plan, const double *grad_dev, int64_t grad_stride, const double *coef_dev,
                                        const double *scale_dev, int n_cand, double *out_dev, int64_t out_stride, void *stream)
{
    int rc = plan_ready(plan, n_cand); if (rc) return rc;
    if (!grad_dev || !coef_dev || !out_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    const int n_out = (int)plan->outs.size();
    hipLaunchKernelGGL(k_combine_grad, dim3((unsigned)((plan->L + 255) / 256), n_cand), dim3(256), 0, (hipStream_t)stream, grad_dev,
                       grad_stride, plan->d_goff, plan->d_invmap, plan->L, n_out, coef_dev, scale_dev, n_cand, out_dev, out_stride, plan->gate);
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}


// mlmc.hip -- Part 9 of include/bluest_hip.h: the MLMC model-subset search (bluest/blue_models.py:642-741 with the allocation of
// bluest/misc.py:15-46 and the brute-force rounding of misc.py:141-167, 384-413).
//
// Positions 0..nb are the models in decreasing cost order, model 0 first.  A group is a bitmask over positions 1..nb; its models
// are position 0 and the kept positions in increasing order, and it is admissible when consecutive models are coupled (a path).
// Level i of a group couples g_i with g_{i+1} (variance lv[n][g_i][g_{i+1}], cost w[g_i] + w[g_{i+1}]); the last level is
// g_{L-1} alone.  The reference takes the argmin over admissible groups ([0] first, then by decreasing size, then by the removed
// positions in lexicographic order, strict "<") of
//   eps mode:    the MODEL costs w[g_i] times the element-wise maximum over outputs of the per-output samples,
//   budget mode: the largest error over outputs.
// The continuous relaxation costs O(L) per group and output and is one scan.  The integer mode is made cheap by bounds: every
// entry the rounding can choose is the floor or the ceil of the continuous one, and a left-to-right sum of non-negative terms
// is monotone in each of them in IEEE arithmetic.  So the objective at all-floor (eps) / all-ceil (budget) is a lower bound LB,
// and the one at all-ceil / all-floor -- a combination the rounding tries -- an upper bound UB where it passes every output's
// constraint; no slack is needed.  Only groups with LB <= min UB are rounded, one workgroup each, over windows of increasing LB.
//
// Arithmetic follows the reference expression by expression (float64, no contraction, sums left to right) so that feasibility
// and rounding decide the same way.
#include "subset_search.hpp"

#pragma clang fp contract(off)

namespace {

using subset_search::BLK;
using subset_search::CAND_CAP;
using subset_search::atomic_min_pos;
using subset_search::atomic_max_pos;

constexpr int MAXL = BLUEST_MLMC_MAX_CANDIDATES + 1;       // models in a group, model 0 included

struct Prob {
    int nb, n_out, budget_mode, continuous;
    double budget;
    const double *w;        // nb+1 model costs by position
    const double *lv;       // n_out x (nb+1) x (nb+1) level variances
    const double *eps2;     // n_out: eps**2
    const uint32_t *adj;    // nb+1: bit q set when positions p and q are coupled
};

// the reference's enumeration: [0] alone, then by decreasing size, then the removed positions in lexicographic order
struct GroupOrder {
    static __device__ __forceinline__ bool before(uint32_t a, uint32_t b)
    {
        if (a == b) return false;
        if (a == 0u || b == 0u) return a == 0u;
        const int pa = __popc(a), pb = __popc(b);
        if (pa != pb) return pa > pb;
        const uint32_t d = a ^ b;
        return (a & (d & (0u - d))) == 0u;
    }
};

__device__ __forceinline__ bool better(double fa, uint32_t ma, double fb, uint32_t mb)
{
    return subset_search::better<GroupOrder>(fa, ma, fb, mb);
}

// consecutive models coupled (blue_models.py:669)
__device__ __forceinline__ bool is_path(const Prob &P, uint32_t mask)
{
    int p = 0;
    for (uint32_t rest = mask; rest; rest &= rest - 1) {
        const int q = __builtin_ctz(rest) + 1;
        if (!((P.adj[p] >> q) & 1u)) return false;
        p = q;
    }
    return true;
}

// f(i, v_i, c_i, w[g_i]) for the levels of output n of a group, in order
template <typename F>
__device__ __forceinline__ void for_levels(const Prob &P, uint32_t mask, int n, F f)
{
    const int M1 = P.nb + 1;
    const double *lv = P.lv + (int64_t)n * M1 * M1;
    int p = 0, i = 0;
    for (uint32_t rest = mask; rest; rest &= rest - 1) {
        const int q = __builtin_ctz(rest) + 1;
        f(i, lv[p * M1 + q], P.w[p] + P.w[q], P.w[p]);
        p = q; i++;
    }
    f(i, lv[p * M1 + p], P.w[p], P.w[p]);
}

// misc.py:21-25: false when a level variance is not finite; mu = budget/q or q/eps**2
__device__ __forceinline__ bool level_mu(const Prob &P, uint32_t mask, int n, double &mu)
{
    bool finite = true;
    double q = 0.0;
    for_levels(P, mask, n, [&](int, double v, double c, double) { finite = finite && isfinite(v); q += sqrt(v * c); });
    mu = P.budget_mode ? P.budget / q : q / P.eps2[n];
    return finite;
}

// misc.py:26-27: np.maximum keeps a NaN
__device__ __forceinline__ double m_cont(double mu, double v, double c)
{
    const double m = mu * sqrt(v / c);
    return m != m ? m : fmax(m, 1.0);
}

enum { ROUND_NONE = 0, ROUND_FLOOR = 1, ROUND_CEIL = 2 };

// per-thread LDS column of the scan: per level, the maximum over outputs of the samples (eps mode)
struct ScanLds {
    double mx[MAXL * BLK];
    double redf[BLK / WAVE];
    uint32_t redm[BLK / WAVE];
};

// what one group contributes to the scan.  Continuous mode: obj.  Integer mode: lb, ub; big = more than 24 levels to round.
struct GroupEval { bool ok; double obj, lb, ub; bool big; };

// The group objective with every sample of every output rounded one way.  feasible: every level variance finite (and, for a
// rounded sweep, every sample a number); passes: every output's constraint holds at this point.
__device__ double sweep(const Prob &P, uint32_t mask, int rounding, double *mx, bool &feasible, bool &passes)
{
    const bool eps_mode = !P.budget_mode;
    const int L = __popc(mask) + 1;
    feasible = passes = true;
    if (eps_mode) for (int i = 0; i < L; i++) mx[i * BLK] = 0.0;
    double worst = 0.0;
    for (int n = 0; n < P.n_out; n++) {
        double mu;
        if (!level_mu(P, mask, n, mu)) { feasible = false; return INFINITY; }
        double var = 0.0, cost = 0.0;
        bool nan = false;
        for_levels(P, mask, n, [&](int i, double v, double c, double) {
            double m = m_cont(mu, v, c);
            if (rounding == ROUND_FLOOR) m = floor(m);
            if (rounding == ROUND_CEIL) m = ceil(m);
            nan = nan || m != m;
            if (m > 0.0) var += v / m;                                  // variance = sum(v[m>0]/m[m>0])
            cost += m * c;
            if (eps_mode) mx[i * BLK] = (m > mx[i * BLK] || m != m) ? m : mx[i * BLK];
        });
        if (rounding != ROUND_NONE && nan) { feasible = false; return INFINITY; }     // no comparison holds for a NaN
        if (eps_mode) passes = passes && var <= P.eps2[n];
        else {
            passes = passes && cost <= P.budget;
            const double err = sqrt(var);
            worst = (err > worst || err != err) ? err : worst;
        }
    }
    double obj = worst;
    if (eps_mode) {                                                     // model costs, not level costs (blue_models.py:718)
        obj = 0.0;
        for_levels(P, mask, 0, [&](int i, double, double, double wm) { obj += mx[i * BLK] * wm; });
    }
    return obj != obj ? INFINITY : obj;                                 // NaN never wins a strict "<"
}

__device__ GroupEval eval_group(const Prob &P, uint32_t mask, ScanLds &S, int tid, bool want_ub)
{
    GroupEval E{false, INFINITY, INFINITY, INFINITY, false};
    if (!is_path(P, mask)) return E;
    double *mx = S.mx + tid;
    bool feasible, passes;
    if (P.continuous) {
        E.obj = sweep(P, mask, ROUND_NONE, mx, feasible, passes);
        E.ok = feasible;
        return E;
    }
    if (__popc(mask) + 1 > BLUEST_MLMC_MAX_ROUND) {                     // the reference raises once output 0 gets to the rounding
        double mu;
        E.big = level_mu(P, mask, 0, mu);
        return E;
    }
    E.lb = sweep(P, mask, P.budget_mode ? ROUND_CEIL : ROUND_FLOOR, mx, feasible, passes);
    if (!feasible) { E.lb = INFINITY; return E; }
    E.ok = true;
    if (want_ub) {
        const double ub = sweep(P, mask, P.budget_mode ? ROUND_FLOOR : ROUND_CEIL, mx, feasible, passes);
        if (feasible && passes) E.ub = ub;
    }
    return E;
}

// pass 0 (continuous): per-block best group.  pass 1 (integer): min UB, max finite LB, the > 24 flag.
// pass 2 (integer): count groups with lo < LB <= hi.  pass 3: collect them (first CAND_CAP).
__global__ __launch_bounds__(BLK) void k_mlmc_scan(Prob P, int pass, uint64_t total, double lo, double hi, double *partf,
                                                   uint32_t *partm, double *stats, unsigned long long *count, uint32_t *cand)
{
    __shared__ ScanLds S;
    const int tid = threadIdx.x;
    double bf = INFINITY, ub = INFINITY, lbm = 0.0;
    uint32_t bm = 0xffffffffu;
    bool big = false;
    for (uint64_t mask = (uint64_t)blockIdx.x * BLK + tid; mask < total; mask += (uint64_t)gridDim.x * BLK) {
        const GroupEval E = eval_group(P, (uint32_t)mask, S, tid, pass == 1);
        big |= E.big;
        if (!E.ok) continue;
        if (pass == 0) {
            if (better(E.obj, (uint32_t)mask, bf, bm)) { bf = E.obj; bm = (uint32_t)mask; }
        } else if (pass == 1) {
            ub = fmin(ub, E.ub);
            if (E.lb < INFINITY) lbm = fmax(lbm, E.lb);
        } else if (E.lb > lo && E.lb <= hi) {
            const unsigned long long k = atomicAdd(count, 1ull);
            if (pass == 3 && k < (unsigned long long)CAND_CAP) cand[k] = (uint32_t)mask;
        }
    }
    if (pass == 0) {
        subset_search::block_best<GroupOrder>(bf, bm, S.redf, S.redm, tid);
        if (tid == 0) { partf[blockIdx.x] = bf; partm[blockIdx.x] = bm; }
    } else if (pass == 1) {
        ub = wave_min(ub);
        lbm = wave_max(lbm);
        const bool anybig = __any(big);
        if ((tid & 63) == 0) {
            if (ub < INFINITY) atomic_min_pos(&stats[0], ub);
            atomic_max_pos(&stats[1], lbm);
            if (anybig) atomic_max_pos(&stats[2], 1.0);
        }
    }
}

// the brute-force rounding of misc.py:384-413 for one candidate group per workgroup, every output; writes the group objective
// and the chosen combination index per output
struct RoundLds {
    double lb[MAXL], ub[MAXL], vlb[MAXL], vub[MAXL], cl[MAXL], wm[MAXL], mx[MAXL];
    int jbit[MAXL];
    int L;
    double redf[BLK / WAVE];
    uint32_t redc[BLK / WAVE];
    double fval[BLUEST_MLMC_MAX_OUTPUTS];
    uint32_t combo[BLUEST_MLMC_MAX_OUTPUTS];
};

__global__ __launch_bounds__(BLK) void k_mlmc_round(Prob P, const uint32_t *cand, double *cobj, uint32_t *ccombo)
{
    __shared__ RoundLds R;
    const int tid = threadIdx.x;
    const uint32_t mask = cand[blockIdx.x];
    const bool eps_mode = !P.budget_mode;
    const int L = __popc(mask) + 1;                                     // <= BLUEST_MLMC_MAX_ROUND: the scan lists no larger group
    for (int n = 0; n < P.n_out; n++) {
        if (tid == 0) {
            double mu, m[MAXL];
            level_mu(P, mask, n, mu);
            for_levels(P, mask, n, [&](int i, double v, double c, double wm) {
                m[i] = m_cont(mu, v, c);
                R.lb[i] = floor(m[i]); R.ub[i] = ceil(m[i]);
                R.vlb[i] = v / R.lb[i]; R.vub[i] = v / R.ub[i];
                R.cl[i] = c; R.wm[i] = wm;
            });
            // get_feasible_integer_bounds: idx = argsort(sol) (ascending, ties by position), then argsort(lb[idx])[::-1]
            int idx[MAXL], ord2[MAXL];
            for (int i = 0; i < L; i++) {
                int j = i;
                while (j > 0 && m[idx[j - 1]] > m[i]) { idx[j] = idx[j - 1]; j--; }
                idx[j] = i;
            }
            for (int i = 0; i < L; i++) {
                int j = i;
                while (j > 0 && R.lb[idx[ord2[j - 1]]] > R.lb[idx[i]]) { ord2[j] = ord2[j - 1]; j--; }
                ord2[j] = i;
            }
            for (int j = 0; j < L; j++) R.jbit[idx[ord2[L - 1 - j]]] = j;
            if (n == 0) for (int i = 0; i < L; i++) R.mx[i] = 0.0;
        }
        __syncthreads();
        const double e2 = eps_mode ? P.eps2[n] : 0.0;
        double bf = INFINITY;
        uint32_t bc = 0xffffffffu;
        for (uint32_t c = tid; c < (1u << L); c += BLK) {
            double cost = 0.0, var = 0.0;
            for (int i = 0; i < L; i++) {
                const bool up = (c >> R.jbit[i]) & 1u;
                var += up ? R.vub[i] : R.vlb[i];
                cost += (up ? R.ub[i] : R.lb[i]) * R.cl[i];
            }
            double f;
            if (P.budget_mode) f = cost <= P.budget ? var : INFINITY;
            else f = var <= e2 ? cost : INFINITY;
            if (f < bf) { bf = f; bc = c; }                             // increasing c per thread: first minimum kept
        }
        for (int off = 32; off > 0; off >>= 1) {
            const double of = __shfl_xor(bf, off, WAVE);
            const uint32_t oc = __shfl_xor(bc, off, WAVE);
            if (of < bf || (of == bf && oc < bc)) { bf = of; bc = oc; }
        }
        if ((tid & 63) == 0) { R.redf[tid >> 6] = bf; R.redc[tid >> 6] = bc; }
        __syncthreads();
        if (tid == 0) {
            for (int k = 1; k < BLK / WAVE; k++)
                if (R.redf[k] < bf || (R.redf[k] == bf && R.redc[k] < bc)) { bf = R.redf[k]; bc = R.redc[k]; }
            R.fval[n] = bf;
            R.combo[n] = bf < INFINITY ? bc : 0u;
            if (eps_mode && bf < INFINITY)
                for (int i = 0; i < L; i++) R.mx[i] = fmax(R.mx[i], ((bc >> R.jbit[i]) & 1u) ? R.ub[i] : R.lb[i]);
        }
        __syncthreads();
    }
    if (tid == 0) {
        double obj = 0.0;
        bool ok = true;
        for (int n = 0; n < P.n_out; n++) ok = ok && R.fval[n] < INFINITY;
        if (ok && eps_mode) {
            for (int i = 0; i < L; i++) obj += R.mx[i] * R.wm[i];
        } else if (ok) {
            for (int n = 0; n < P.n_out; n++) { const double e = sqrt(R.fval[n]); obj = (e > obj || e != e) ? e : obj; }
        }
        if (!ok || obj != obj) obj = INFINITY;
        cobj[blockIdx.x] = obj;
        for (int n = 0; n < P.n_out; n++) ccombo[(int64_t)blockIdx.x * P.n_out + n] = R.combo[n];
    }
}

constexpr auto k_mlmc_pick = subset_search::k_pick<GroupOrder>;

}  // namespace

// ------------------------------------------------------------------------------------------------------
// MLMC model-subset search
// ------------------------------------------------------------------------------------------------------
extern "C" int bluest_mlmc_search(int nb, int n_out, int flags, double budget, const double *eps2, const double *w, const double *lv,
                                  const uint32_t *adj, uint32_t *best_mask, uint32_t *best_combo, double *best_obj,
                                  int32_t *status, void *stream)
{
    int rc = require_gpu(); if (rc) return rc;
    if (nb < 0 || nb > BLUEST_MLMC_MAX_CANDIDATES) return fail(BLUEST_ERR_ARG, "nb=%d out of range (0..%d)", nb, BLUEST_MLMC_MAX_CANDIDATES);
    if (n_out <= 0 || n_out > BLUEST_MLMC_MAX_OUTPUTS) return fail(BLUEST_ERR_ARG, "n_out=%d out of range", n_out);
    if (!w || !lv || !adj || !best_mask || !best_combo || !best_obj || !status) return fail(BLUEST_ERR_ARG, "null pointer");
    const bool budget_mode = (flags & BLUEST_MLMC_BUDGET) != 0;
    if (!budget_mode && !eps2) return fail(BLUEST_ERR_ARG, "eps mode needs eps2");
    hipStream_t st = (hipStream_t)stream;
    const int M1 = nb + 1;
    Prob P;
    P.nb = nb; P.n_out = n_out; P.budget_mode = budget_mode;
    P.continuous = (flags & BLUEST_MLMC_CONTINUOUS) != 0;
    P.budget = budget;

    // one device block: tables, then work arrays
    const uint64_t total = 1ull << nb;
    const int grid = (int)std::min<uint64_t>((total + BLK - 1) / BLK, 4096);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_w = take(M1 * 8), o_lv = take((size_t)n_out * M1 * M1 * 8), o_e2 = take(n_out * 8), o_a = take(M1 * 4);
    const size_t o_pf = take(grid * 8), o_pm = take(grid * 4), o_st = take(3 * 8), o_cnt = take(8), o_cand = take(CAND_CAP * 4);
    const size_t o_cobj = take(CAND_CAP * 8), o_cc = take((size_t)CAND_CAP * n_out * 4);
    const size_t o_bf = take(8), o_bm = take(4), o_bc = take(n_out * 4);
    char *d = nullptr;
    HIP_TRY(hipMalloc(&d, off));
    struct Free { char *p; ~Free() { if (p) (void)hipFree(p); } } guard{d};
    auto up = [&](size_t o, const void *h, size_t bytes) { return hipMemcpyAsync(d + o, h, bytes, hipMemcpyHostToDevice, st); };
    HIP_TRY(up(o_w, w, M1 * 8));
    HIP_TRY(up(o_lv, lv, (size_t)n_out * M1 * M1 * 8));
    if (!budget_mode) HIP_TRY(up(o_e2, eps2, n_out * 8));
    HIP_TRY(up(o_a, adj, M1 * 4));
    P.w = (const double *)(d + o_w); P.lv = (const double *)(d + o_lv); P.eps2 = (const double *)(d + o_e2);
    P.adj = (const uint32_t *)(d + o_a);
    double *partf = (double *)(d + o_pf), *stats = (double *)(d + o_st), *cobj = (double *)(d + o_cobj), *bf = (double *)(d + o_bf);
    uint32_t *partm = (uint32_t *)(d + o_pm), *cand = (uint32_t *)(d + o_cand), *cc = (uint32_t *)(d + o_cc);
    uint32_t *bm = (uint32_t *)(d + o_bm), *bc = (uint32_t *)(d + o_bc);
    unsigned long long *cnt = (unsigned long long *)(d + o_cnt);
    const double inf = INFINITY;
    const uint32_t none = 0xffffffffu;
    HIP_TRY(hipMemcpyAsync(bf, &inf, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bm, &none, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(bc, 0, n_out * 4, st));

    if (P.continuous) {
        hipLaunchKernelGGL(k_mlmc_scan, dim3(grid), dim3(BLK), 0, st, P, 0, total, 0.0, 0.0, partf, partm, stats, cnt, cand);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mlmc_pick, dim3(1), dim3(BLK), 0, st, (int64_t)grid, (const double *)partf, (const uint32_t *)partm,
                           (const uint32_t *)nullptr, (const uint32_t *)nullptr, n_out, bf, bm, bc);
        HIP_TRY(hipGetLastError());
    } else {
        const double st0[3] = {INFINITY, 0.0, 0.0};
        HIP_TRY(hipMemcpyAsync(stats, st0, 24, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mlmc_scan, dim3(grid), dim3(BLK), 0, st, P, 1, total, 0.0, 0.0, partf, partm, stats, cnt, cand);
        HIP_TRY(hipGetLastError());
        double hs[3];
        HIP_TRY(hipMemcpyAsync(hs, stats, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hs[2] > 0.0) { *status = BLUEST_MLMC_TOO_BIG; return BLUEST_OK; }
        auto count_in = [&](bool collect, double a, double b, unsigned long long *out) -> int {
            HIP_TRY(hipMemsetAsync(cnt, 0, 8, st));
            hipLaunchKernelGGL(k_mlmc_scan, dim3(grid), dim3(BLK), 0, st, P, collect ? 3 : 2, total, a, b, partf, partm, stats, cnt,
                               cand);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(out, cnt, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return BLUEST_OK;
        };
        auto round_them = [&](unsigned long long c, double *best) -> int {
            hipLaunchKernelGGL(k_mlmc_round, dim3((unsigned)c), dim3(BLK), 0, st, P, (const uint32_t *)cand, cobj, cc);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_mlmc_pick, dim3(1), dim3(BLK), 0, st, (int64_t)c, (const double *)cobj,
                               (const uint32_t *)nullptr, (const uint32_t *)cand, (const uint32_t *)cc, n_out, bf, bm, bc);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(best, bf, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return BLUEST_OK;
        };
        if ((rc = subset_search::window_loop(hs[0], hs[1], "group", count_in, round_them))) return rc;
    }
    double hobj;
    HIP_TRY(hipMemcpyAsync(&hobj, bf, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(best_mask, bm, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(best_combo, bc, n_out * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    *best_obj = hobj;
    *status = hobj < INFINITY ? BLUEST_MLMC_OK : BLUEST_MLMC_NONE;
    return BLUEST_OK;
}

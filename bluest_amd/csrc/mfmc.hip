// mfmc.hip -- Part 7 of include/bluest_hip.h: the MFMC model-subset search (bluest/blue_models.py:795-865 with the allocation of
// bluest/misc.py:78-130 and the brute-force rounding of misc.py:141-175, 384-413 / the low-budget scheme of misc.py:416-449).
//
// A candidate subset is a bitmask over the neighbours of model 0 in the intersection of the coupling graphs.  The reference takes
// the argmin over cliques (size first, then lexicographic: networkx.enumerate_all_cliques order, strict "<") of
//   eps mode:    cost of the element-wise maximum over outputs of the per-output rounded samples,
//   budget mode: the largest error over outputs.
// Exact modes (continuous_relaxation, or small_budget with a budget) cost O(L) per clique and are evaluated in one scan.  The
// integer mode is made cheap by bounds: with the variance written as s0^2 [(1-r1^2)/m0 + sum_i (r_i^2 - r_{i+1}^2)/m_i] the
// closed-form optimum of the relaxed problem is a lower bound LB of any integer point, and the all-ceil (eps) / all-floor
// (budget) combination -- one of the 2^L the rounding tries -- is an upper bound UB where feasible.  Only cliques with
// LB <= min UB are rounded, one workgroup each, over windows of increasing LB.
//
// Arithmetic follows the reference expression by expression (float64, no contraction) so that feasibility and rounding decide
// the same way.
#include "subset_search.hpp"

#pragma clang fp contract(off)

namespace {

using subset_search::BLK;
using subset_search::CAND_CAP;
using subset_search::atomic_min_pos;
using subset_search::atomic_max_pos;
constexpr int MAXL = BLUEST_MFMC_MAX_NEIGHBOURS + 1;      // models in a clique, model 0 included
// Relative slack of the lower bound.  The reference's variance sum s0^2/m0 + sum (1/m_{i-1} - 1/m_i) c_i cancels down to at least
// s0^2 (1 - rho_1^2)/m0, and its terms are at most ~3 s0^2/m0 in size.  Its rounding error relative to the result is therefore
// below ~8 L eps / (1 - rho_1^2).  A point the reference accepts (var <= eps^2, or cost <= budget) can beat the exact relaxed
// optimum by at most that much, so the lower bound is taken that much lower (never below 1e-9, never below zero).
constexpr double LB_MARGIN_MIN = 1e-9;
constexpr double LB_MARGIN_ULPS = 16.0;
struct Prob {
    int nb, n_out, budget_mode, continuous, small_budget, integer_round;
    double budget;
    const double *w;        // nb+1, local index 0 = model 0, p = neighbour p-1
    const double *s;        // n_out x (nb+1) standard deviations
    const double *rho;      // n_out x (nb+1) correlations with model 0
    const double *eps2;     // n_out: eps**2
    const double *epsm2;    // n_out: eps**-2
    const int32_t *perm;    // n_out x (nb+1): local indices by decreasing |rho| (model 0 first)
    const uint32_t *adj;    // nb: neighbour bitmask of each neighbour
};

__device__ __forceinline__ bool in_clique(uint32_t mask, int q) { return q == 0 || ((mask >> (q - 1)) & 1u); }

__device__ __forceinline__ bool is_clique(const Prob &P, uint32_t mask)
{
    for (uint32_t rest = mask; rest; rest &= rest - 1) {
        const int b = __builtin_ctz(rest);
        if ((mask & ~(P.adj[b] | (1u << b))) != 0u) return false;
    }
    return true;
}

// enumeration order of networkx.enumerate_all_cliques for cliques through model 0: size, then lexicographic
struct CliqueOrder {
    static __device__ __forceinline__ bool before(uint32_t a, uint32_t b)
    {
        const int pa = __popc(a), pb = __popc(b);
        if (pa != pb) return pa < pb;
        const uint32_t d = a ^ b;
        return d != 0u && ((a & (d & (0u - d))) != 0u);
    }
};

__device__ __forceinline__ bool better(double fa, uint32_t ma, double fb, uint32_t mb)
{
    return subset_search::better<CliqueOrder>(fa, ma, fb, mb);
}

// one output of one clique: its models in |rho| order (per-thread column of LDS)
struct View {
    const Prob &P;
    int n, L;
    uint8_t *ord;           // ord[i * BLK]
    __device__ View(const Prob &P_, int n_, uint32_t mask, uint8_t *col) : P(P_), n(n_), L(0), ord(col)
    {
        const int32_t *pm = P.perm + (int64_t)n * (P.nb + 1);
        for (int r = 0; r <= P.nb; r++) {
            const int q = pm[r];
            if (in_clique(mask, q)) { ord[L * BLK] = (uint8_t)q; L++; }
        }
    }
    __device__ int q(int i) const { return ord[i * BLK]; }
    __device__ double rho(int i) const { return i < L ? P.rho[(int64_t)n * (P.nb + 1) + q(i)] : 0.0; }
    __device__ double sig(int i) const { return P.s[(int64_t)n * (P.nb + 1) + q(i)]; }
    __device__ double w(int i) const { return P.w[q(i)]; }

    // misc.py:96-99: all(w[:-1]/w[1:] > (rho[:-2]**2 - rho[1:-1]**2)/(rho[1:-1]**2 - rho[2:]**2))
    __device__ bool feasible() const
    {
        for (int i = 0; i + 1 < L; i++) {
            const double a = rho(i), b = rho(i + 1), c = rho(i + 2);
            const double cr = w(i) / w(i + 1);
            const double rr = (a * a - b * b) / (b * b - c * c);
            if (!(cr > rr)) return false;
        }
        return true;
    }
    // misc.py:103: r = sqrt(w[0]/w*(rho[:-1]**2 - rho[1:]**2)/(1-rho[1]**2))
    __device__ double r(int i) const
    {
        const double a = rho(i), b = rho(i + 1), r1 = rho(1);
        return sqrt(((w(0) / w(i)) * (a * a - b * b)) / (1.0 - r1 * r1));
    }
    // misc.py:104-106, unclamped
    __device__ double m1() const
    {
        double dot = 0.0;
        for (int i = 0; i < L; i++) dot += w(i) * r(i);
        if (P.budget_mode) return P.budget / dot;
        const double s0 = sig(0), r1 = rho(1);
        return ((P.epsm2[n] * dot) * ((s0 * s0) / w(0))) * (1.0 - r1 * r1);
    }
    __device__ double m_cont(double m1v, int i) const { return fmax(i == 0 ? m1v : m1v * r(i), 1.0); }   // np.maximum(m, 1)
    // misc.py:93 coefficient: alphas**2*s[1:]**2 - 2*alphas*rho[1:-1]*s[0]*s[1:]
    __device__ double coef(int i) const
    {
        const double s0 = sig(0), si = sig(i), ri = rho(i);
        const double al = (ri * s0) / si;
        return (al * al) * (si * si) - (((2.0 * al) * ri) * s0) * si;
    }
    // closed-form optimum of the relaxed problem: Q = sum sqrt(a_i w_i), a_0 = 1 - rho_1^2, a_i = rho_i^2 - rho_{i+1}^2
    __device__ double lower_bound() const
    {
        double Q = 0.0;
        for (int i = 0; i < L; i++) {
            const double a = i == 0 ? 1.0 - rho(1) * rho(1) : rho(i) * rho(i) - rho(i + 1) * rho(i + 1);
            Q += sqrt(fmax(a, 0.0) * w(i));
        }
        const double s0 = sig(0), r1 = rho(1);
        const double v = P.budget_mode ? sqrt((s0 * s0) * (Q * Q) / P.budget) : (Q * Q) * (s0 * s0) / P.eps2[n];
        const double margin = fmax(LB_MARGIN_MIN, LB_MARGIN_ULPS * L * __DBL_EPSILON__ / (1.0 - r1 * r1));
        return margin < 1.0 ? v * (1.0 - margin) : 0.0;     // |rho_1| = 1: infinite margin, no pruning
    }
};

// variance(m) of misc.py:117 for m given position by position through `mat(i)`
template <typename F>
__device__ __forceinline__ double variance(const View &V, F mat)
{
    const double s0 = V.sig(0);
    double sum = 0.0, prev = mat(0);
    for (int i = 1; i < V.L; i++) {
        const double mi = mat(i);
        sum += (1.0 / prev - 1.0 / mi) * V.coef(i);
        prev = mi;
    }
    return (s0 * s0) / mat(0) + sum;
}

// misc.py:416-449 on the clique in |rho| order; writes m into mcol[i * BLK]
__device__ void low_budget(const View &V, double budget, double *mcol)
{
    int start = 0;
    while (true) {
        const int Ls = V.L - start;
        if (Ls == 1) { mcol[start * BLK] = floor(budget / V.w(start)); return; }
        const double r0 = V.rho(start), r1 = V.rho(start + 1);
        const double denom = r0 * r0 - r1 * r1;
        double dot = 0.0;
        for (int i = start; i < V.L; i++) {
            const double a = V.rho(i), b = V.rho(i + 1);
            dot += V.w(i) * sqrt(((V.w(start) / V.w(i)) * (a * a - b * b)) / denom);
        }
        const double m1 = budget / dot;
        if (m1 >= 1.0) {
            for (int i = start; i < V.L; i++) {
                const double a = V.rho(i), b = V.rho(i + 1);
                const double ri = sqrt(((V.w(start) / V.w(i)) * (a * a - b * b)) / denom);
                mcol[i * BLK] = floor(i == start ? m1 : m1 * ri);
            }
            return;
        }
        mcol[start * BLK] = 1.0;
        budget = budget - V.w(start);
        start++;
    }
}

// per-thread LDS columns of the scan
struct ScanLds {
    uint8_t ord[MAXL * BLK];
    union {
        double mx[MAXL * BLK];      // eps mode: per local model, max over outputs
        double mpos[MAXL * BLK];    // small_budget (budget mode): per position, the low-budget allocation
    };
    double redf[BLK / WAVE];
    uint32_t redm[BLK / WAVE];
};

// what one clique contributes to the scan.  Exact modes: obj.  Integer mode: lb, ub; big = needs > 24 rounding dimensions.
struct CliqueEval { bool ok; double obj, lb, ub; bool big; };

__device__ CliqueEval eval_clique(const Prob &P, uint32_t mask, ScanLds &S, int tid)
{
    CliqueEval E{false, INFINITY, INFINITY, INFINITY, false};
    if (!is_clique(P, mask)) return E;
    uint8_t *col = S.ord + tid;
    double *mx = S.mx + tid;
    const bool eps_mode = !P.budget_mode;
    if (eps_mode) for (int q = 0; q <= P.nb; q++) mx[q * BLK] = 0.0;
    double worst = 0.0, lbmax = 0.0;
    bool ub_ok = true;
    for (int n = 0; n < P.n_out; n++) {
        View V(P, n, mask, col);
        if (!V.feasible()) return E;
        if (P.integer_round && V.L > BLUEST_MFMC_MAX_ROUND) { E.big = true; return E; }
        const double m1 = V.m1();
        if (P.integer_round) {
            lbmax = fmax(lbmax, V.lower_bound());
            if (!ub_ok) continue;
            // all-ceil (eps) / all-floor (budget) combination
            auto mr = [&](int i) { const double m = V.m_cont(m1, i); return P.budget_mode ? floor(m) : ceil(m); };
            bool ok = mr(0) >= 1.0;
            double cost = 0.0;
            for (int i = 0; i < V.L && ok; i++) {
                if (i > 0 && !(mr(i - 1) <= mr(i))) ok = false;
                cost += mr(i) * V.w(i);
            }
            if (ok && P.budget_mode) ok = cost <= P.budget;
            const double var = ok ? variance(V, mr) : INFINITY;
            if (ok && eps_mode) ok = var <= P.eps2[n];
            if (!ok) { ub_ok = false; continue; }
            if (eps_mode) for (int i = 0; i < V.L; i++) mx[V.q(i) * BLK] = fmax(mx[V.q(i) * BLK], mr(i));
            else worst = fmax(worst, sqrt(var));
        } else if (P.budget_mode && P.small_budget) {
            double *mp = S.mpos + tid;
            low_budget(V, P.budget, mp);
            const double err = sqrt(variance(V, [&](int i) { return mp[i * BLK]; }));
            worst = (err > worst || err != err) ? err : worst;
        } else {                                                        // continuous relaxation
            auto mc = [&](int i) { return V.m_cont(m1, i); };
            if (eps_mode) for (int i = 0; i < V.L; i++) mx[V.q(i) * BLK] = fmax(mx[V.q(i) * BLK], mc(i));
            else {
                const double err = sqrt(variance(V, mc));
                worst = (err > worst || err != err) ? err : worst;
            }
        }
    }
    double obj = worst;
    if (eps_mode && (ub_ok || !P.integer_round)) {                      // cost of the per-model maximum, in output 0's order
        View V(P, 0, mask, col);
        obj = 0.0;
        for (int i = 0; i < V.L; i++) obj += mx[V.q(i) * BLK] * V.w(i);
    }
    if (obj != obj) obj = INFINITY;                                     // NaN never wins a strict "<"
    E.ok = true;
    if (P.integer_round) { E.lb = lbmax; E.ub = ub_ok ? obj : INFINITY; }
    else E.obj = obj;
    return E;
}

// pass 0 (exact modes): per-block best clique.  pass 1 (integer): min UB, max finite LB, the > 24 flag.
// pass 2 (integer): count cliques with lo < LB <= hi.  pass 3: collect them (first CAND_CAP).
__global__ __launch_bounds__(BLK) void k_mfmc_scan(Prob P, int pass, uint64_t total, double lo, double hi, double *partf,
                                                   uint32_t *partm, double *stats, unsigned long long *count, uint32_t *cand)
{
    __shared__ ScanLds S;
    const int tid = threadIdx.x;
    double bf = INFINITY, ub = INFINITY, lbm = 0.0;
    uint32_t bm = 0xffffffffu;
    bool big = false;
    for (uint64_t mask = (uint64_t)blockIdx.x * BLK + tid; mask < total; mask += (uint64_t)gridDim.x * BLK) {
        const CliqueEval E = eval_clique(P, (uint32_t)mask, S, tid);
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
        subset_search::block_best<CliqueOrder>(bf, bm, S.redf, S.redm, tid);
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

// the brute-force rounding of misc.py:384-413 for one candidate clique per workgroup, every output; writes the clique objective
// and the chosen combination index per output
struct RoundLds {
    uint8_t ord[MAXL * BLK];    // View needs a column; only thread 0's is used
    double lb[MAXL], ub[MAXL], ilb[MAXL], iub[MAXL], cf[MAXL], wv[MAXL], mx[MAXL];
    int jbit[MAXL];
    double s0;
    int L;
    double redf[BLK / WAVE];
    uint32_t redc[BLK / WAVE];
    double fval[BLUEST_MFMC_MAX_OUTPUTS];
    uint32_t combo[BLUEST_MFMC_MAX_OUTPUTS];
};

__global__ __launch_bounds__(BLK) void k_mfmc_round(Prob P, const uint32_t *cand, double *cobj, uint32_t *ccombo)
{
    __shared__ RoundLds R;
    const int tid = threadIdx.x;
    const uint32_t mask = cand[blockIdx.x];
    const bool eps_mode = !P.budget_mode;
    int L = 0;
    for (int n = 0; n < P.n_out; n++) {
        if (tid == 0) {
            View V(P, n, mask, R.ord);
            L = V.L;
            const double m1 = V.m1();
            int idx[MAXL];
            for (int i = 0; i < L; i++) {
                const double m = V.m_cont(m1, i);
                R.lb[i] = floor(m); R.ub[i] = ceil(m);
                R.ilb[i] = 1.0 / R.lb[i]; R.iub[i] = 1.0 / R.ub[i];
                R.cf[i] = V.coef(i); R.wv[i] = V.w(i);
            }
            R.s0 = V.sig(0);
            // get_feasible_integer_bounds: idx = argsort(sol) (ascending, ties by position), then argsort(lb[idx])[::-1]
            for (int i = 0; i < L; i++) {
                int j = i;
                const double key = V.m_cont(m1, i);
                while (j > 0 && V.m_cont(m1, idx[j - 1]) > key) { idx[j] = idx[j - 1]; j--; }
                idx[j] = i;
            }
            int ord2[MAXL];
            for (int i = 0; i < L; i++) {
                int j = i;
                while (j > 0 && R.lb[idx[ord2[j - 1]]] > R.lb[idx[i]]) { ord2[j] = ord2[j - 1]; j--; }
                ord2[j] = i;
            }
            for (int j = 0; j < L; j++) R.jbit[idx[ord2[L - 1 - j]]] = j;
        }
        if (tid == 0) R.L = L;
        __syncthreads();
        L = R.L;
        const double s0sq = R.s0 * R.s0, e2 = eps_mode ? P.eps2[n] : 0.0;
        double bf = INFINITY;
        uint32_t bc = 0xffffffffu;
        for (uint32_t c = tid; c < (1u << L); c += BLK) {
            double prev = 0.0, iprev = 0.0, cost = 0.0, sum = 0.0, m0 = 0.0;
            bool ok = true;
            for (int i = 0; i < L; i++) {
                const bool up = (c >> R.jbit[i]) & 1u;
                const double mi = up ? R.ub[i] : R.lb[i], imi = up ? R.iub[i] : R.ilb[i];
                if (i == 0) { m0 = mi; ok = mi >= 1.0; }
                else { ok = ok && prev <= mi; sum += (iprev - imi) * R.cf[i]; }
                cost += mi * R.wv[i];
                prev = mi; iprev = imi;
            }
            const double var = s0sq / m0 + sum;
            double f;
            if (P.budget_mode) f = (ok && cost <= P.budget) ? var : INFINITY;
            else f = (ok && var <= e2) ? cost : INFINITY;
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
            if (eps_mode) {
                if (n == 0) for (int q = 0; q < MAXL; q++) R.mx[q] = 0.0;
                View V(P, n, mask, R.ord);
                for (int i = 0; i < L; i++) {
                    const double mi = ((bc >> R.jbit[i]) & 1u) ? R.ub[i] : R.lb[i];
                    R.mx[V.q(i)] = fmax(R.mx[V.q(i)], mi);
                }
            }
        }
        __syncthreads();
    }
    if (tid == 0) {
        double obj = 0.0;
        bool ok = true;
        for (int n = 0; n < P.n_out; n++) ok = ok && R.fval[n] < INFINITY;
        if (ok && eps_mode) {
            View V(P, 0, mask, R.ord);
            for (int i = 0; i < V.L; i++) obj += R.mx[V.q(i)] * V.w(i);
        } else if (ok) {
            for (int n = 0; n < P.n_out; n++) { const double e = sqrt(R.fval[n]); obj = (e > obj || e != e) ? e : obj; }
        }
        if (!ok || obj != obj) obj = INFINITY;
        cobj[blockIdx.x] = obj;
        for (int n = 0; n < P.n_out; n++) ccombo[(int64_t)blockIdx.x * P.n_out + n] = R.combo[n];
    }
}

constexpr auto k_mfmc_pick = subset_search::k_pick<CliqueOrder>;

}  // namespace

// ------------------------------------------------------------------------------------------------------
// MFMC model-subset search
// ------------------------------------------------------------------------------------------------------
extern "C" int bluest_mfmc_search(int nb, int n_out, int flags, double budget, const double *eps2, const double *epsm2,
                                  const double *w, const double *s, const double *rho, const int32_t *perm, const uint32_t *adj,
                                  uint32_t *best_mask, uint32_t *best_combo, double *best_obj, int32_t *status, void *stream)
{
    int rc = require_gpu(); if (rc) return rc;
    if (nb < 0 || nb > BLUEST_MFMC_MAX_NEIGHBOURS) return fail(BLUEST_ERR_ARG, "nb=%d out of range (0..%d)", nb, BLUEST_MFMC_MAX_NEIGHBOURS);
    if (n_out <= 0 || n_out > BLUEST_MFMC_MAX_OUTPUTS) return fail(BLUEST_ERR_ARG, "n_out=%d out of range", n_out);
    if (!w || !s || !rho || !perm || (nb > 0 && !adj) || !best_mask || !best_combo || !best_obj || !status)
        return fail(BLUEST_ERR_ARG, "null pointer");
    const bool budget_mode = (flags & BLUEST_MFMC_BUDGET) != 0;
    if (!budget_mode && (!eps2 || !epsm2)) return fail(BLUEST_ERR_ARG, "eps mode needs eps2 and epsm2");
    for (int n = 0; n < n_out; n++)
        for (int r = 0; r <= nb; r++) {
            const int q = perm[n * (nb + 1) + r];
            if (q < 0 || q > nb || (r == 0) != (q == 0)) return fail(BLUEST_ERR_ARG, "perm[%d][%d]=%d invalid", n, r, q);
        }
    hipStream_t st = (hipStream_t)stream;
    const int M1 = nb + 1;
    Prob P;
    P.nb = nb; P.n_out = n_out; P.budget_mode = budget_mode;
    P.continuous = (flags & BLUEST_MFMC_CONTINUOUS) != 0;
    P.small_budget = (flags & BLUEST_MFMC_SMALL_BUDGET) != 0;
    P.integer_round = !P.continuous && !(P.small_budget && budget_mode);
    P.budget = budget;

    // one device block: tables, then work arrays
    const uint64_t total = 1ull << nb;
    const int grid = (int)std::min<uint64_t>((total + BLK - 1) / BLK, 4096);
    size_t off = 0;
    auto take = [&](size_t bytes) { size_t o = off; off += (bytes + 255) & ~(size_t)255; return o; };
    const size_t o_w = take(M1 * 8), o_s = take((size_t)n_out * M1 * 8), o_r = take((size_t)n_out * M1 * 8);
    const size_t o_e2 = take(n_out * 8), o_em = take(n_out * 8), o_p = take((size_t)n_out * M1 * 4), o_a = take(std::max(nb, 1) * 4);
    const size_t o_pf = take(grid * 8), o_pm = take(grid * 4), o_st = take(3 * 8), o_cnt = take(8), o_cand = take(CAND_CAP * 4);
    const size_t o_cobj = take(CAND_CAP * 8), o_cc = take((size_t)CAND_CAP * n_out * 4);
    const size_t o_bf = take(8), o_bm = take(4), o_bc = take(n_out * 4);
    char *d = nullptr;
    HIP_TRY(hipMalloc(&d, off));
    struct Free { char *p; ~Free() { if (p) (void)hipFree(p); } } guard{d};
    auto up = [&](size_t o, const void *h, size_t bytes) { return hipMemcpyAsync(d + o, h, bytes, hipMemcpyHostToDevice, st); };
    HIP_TRY(up(o_w, w, M1 * 8));
    HIP_TRY(up(o_s, s, (size_t)n_out * M1 * 8));
    HIP_TRY(up(o_r, rho, (size_t)n_out * M1 * 8));
    if (!budget_mode) { HIP_TRY(up(o_e2, eps2, n_out * 8)); HIP_TRY(up(o_em, epsm2, n_out * 8)); }
    HIP_TRY(up(o_p, perm, (size_t)n_out * M1 * 4));
    if (nb > 0) HIP_TRY(up(o_a, adj, nb * 4));
    P.w = (const double *)(d + o_w); P.s = (const double *)(d + o_s); P.rho = (const double *)(d + o_r);
    P.eps2 = (const double *)(d + o_e2); P.epsm2 = (const double *)(d + o_em);
    P.perm = (const int32_t *)(d + o_p); P.adj = (const uint32_t *)(d + o_a);
    double *partf = (double *)(d + o_pf), *stats = (double *)(d + o_st), *cobj = (double *)(d + o_cobj), *bf = (double *)(d + o_bf);
    uint32_t *partm = (uint32_t *)(d + o_pm), *cand = (uint32_t *)(d + o_cand), *cc = (uint32_t *)(d + o_cc);
    uint32_t *bm = (uint32_t *)(d + o_bm), *bc = (uint32_t *)(d + o_bc);
    unsigned long long *cnt = (unsigned long long *)(d + o_cnt);
    const double inf = INFINITY;
    const uint32_t none = 0xffffffffu;
    HIP_TRY(hipMemcpyAsync(bf, &inf, 8, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemcpyAsync(bm, &none, 4, hipMemcpyHostToDevice, st));
    HIP_TRY(hipMemsetAsync(bc, 0, n_out * 4, st));

    *status = BLUEST_MFMC_OK;
    if (!P.integer_round) {
        hipLaunchKernelGGL(k_mfmc_scan, dim3(grid), dim3(BLK), 0, st, P, 0, total, 0.0, 0.0, partf, partm, stats, cnt, cand);
        HIP_TRY(hipGetLastError());
        hipLaunchKernelGGL(k_mfmc_pick, dim3(1), dim3(BLK), 0, st, (int64_t)grid, partf, partm, (const uint32_t *)nullptr,
                           (const uint32_t *)nullptr, n_out, bf, bm, bc);
        HIP_TRY(hipGetLastError());
    } else {
        const double st0[3] = {INFINITY, 0.0, 0.0};
        HIP_TRY(hipMemcpyAsync(stats, st0, 24, hipMemcpyHostToDevice, st));
        hipLaunchKernelGGL(k_mfmc_scan, dim3(grid), dim3(BLK), 0, st, P, 1, total, 0.0, 0.0, partf, partm, stats, cnt, cand);
        HIP_TRY(hipGetLastError());
        double hs[3];
        HIP_TRY(hipMemcpyAsync(hs, stats, 24, hipMemcpyDeviceToHost, st));
        HIP_TRY(hipStreamSynchronize(st));
        if (hs[2] > 0.0) { *status = BLUEST_MFMC_TOO_BIG; return BLUEST_OK; }
        auto count_in = [&](bool collect, double a, double b, unsigned long long *out) -> int {
            HIP_TRY(hipMemsetAsync(cnt, 0, 8, st));
            hipLaunchKernelGGL(k_mfmc_scan, dim3(grid), dim3(BLK), 0, st, P, collect ? 3 : 2, total, a, b, partf, partm, stats, cnt,
                               cand);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(out, cnt, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return BLUEST_OK;
        };
        auto round_them = [&](unsigned long long c, double *best) -> int {
            hipLaunchKernelGGL(k_mfmc_round, dim3((unsigned)c), dim3(BLK), 0, st, P, (const uint32_t *)cand, cobj, cc);
            HIP_TRY(hipGetLastError());
            hipLaunchKernelGGL(k_mfmc_pick, dim3(1), dim3(BLK), 0, st, (int64_t)c, (const double *)cobj,
                               (const uint32_t *)nullptr, (const uint32_t *)cand, (const uint32_t *)cc, n_out, bf, bm, bc);
            HIP_TRY(hipGetLastError());
            HIP_TRY(hipMemcpyAsync(best, bf, 8, hipMemcpyDeviceToHost, st));
            HIP_TRY(hipStreamSynchronize(st));
            return BLUEST_OK;
        };
        if ((rc = subset_search::window_loop(hs[0], hs[1], "clique", count_in, round_them))) return rc;
    }
    HIP_TRY(hipMemcpyAsync(best_obj, bf, 8, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(best_mask, bm, 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipMemcpyAsync(best_combo, bc, n_out * 4, hipMemcpyDeviceToHost, st));
    HIP_TRY(hipStreamSynchronize(st));
    if (!(*best_obj < INFINITY)) *status = BLUEST_MFMC_NONE;
    return BLUEST_OK;
}

// common.hpp -- shared by every translation unit of libbluest_hip.so: error plumbing, HIP_TRY, wavefront reductions.
#pragma once
#include <hip/hip_runtime.h>

#include <algorithm>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>
#include <thread>
#include <atomic>
#include <chrono>
#include <mutex>
#include <type_traits>

#include "bluest_hip.h"

// ---- error plumbing (definitions in runtime.hip) -----------------------------------------------------
int fail(int code, const char *fmt, ...);
int require_gpu();

// compute units and per-workgroup LDS limit of HIP device `dev`, queried once per device (thread-safe; runtime.hip)
struct DeviceProps { int cus; size_t lds_per_wg; };
hipError_t device_props(int dev, DeviceProps *out);

#define HIP_TRY(expr)                                                                                        \
    do {                                                                                                     \
        hipError_t _e = (expr);                                                                              \
        if (_e != hipSuccess)                                                                                \
            return fail(BLUEST_ERR_HIP, "%s failed: %s (%s:%d)", #expr, hipGetErrorString(_e), __FILE__,     \
                        __LINE__);                                                                           \
    } while (0)

// per-group pseudo-inverse launcher (mirrors.hip), also used by the plan's set-up
int launch_group_pinv(const double *dC, int N, int k, int64_t Lk, const int64_t *dg, double *dout, hipStream_t st);
int launch_group_pinv_u8(const double *dC, int N, int k, int64_t Lk, const uint8_t *dg, double *dout, hipStream_t st);

// ------------------------------------------------------------------------------------------------------
// device helpers
// ------------------------------------------------------------------------------------------------------
#define WAVE 64

// The __shfl_xor butterflies below compile to ds_bpermute_b32: two per double and level, six dependent trips through the LDS
// crossbar per reduction.  They stay for callers that may run under divergent control flow.  Where all 64 lanes are evidently
// active, the *_dpp forms further down pair the same lanes in the same order without touching the LDS.
__device__ __forceinline__ double wave_sum(double x)
{   // fixed xor-butterfly: every lane ends with the same, order-independent-of-timing sum
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;
}
__device__ __forceinline__ double wave_max(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmax(x, __shfl_xor(x, off, WAVE));
    return x;
}
__device__ __forceinline__ double wave_min(double x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x = fmin(x, __shfl_xor(x, off, WAVE));
    return x;
}
// The binary exponent e of x (x = f 2^e with 0.5 <= f < 1), and 0 for zero, inf and NaN.  With x the largest |entry| of a block,
// ldexp(a, -e) brings the block to ordinary size exactly, and since pinv(s A) = pinv(A) / s, ldexp(r, -e) carries a pseudo-inverse
// of the scaled block back: the Jacobi pseudo-inverses (mirrors.hip, plan.hip) form squares and products of entries, which
// overflow from 2^512 and vanish below 2^-537 unscaled.  A block whose largest entry lies within 2^-256 .. 2^256 is left as it is
// (e = 0: its squares are safe, and its result keeps the bits it had before the scaling existed).
__device__ __forceinline__ int pow2_exponent(double x)
{
    int e = 0;
    if (x > 0.0 && x < INFINITY) (void)frexp(x, &e);
    return (e > 256 || e < -256) ? e : 0;
}
__device__ __forceinline__ long long wave_sum_ll(long long x)
{
#pragma unroll
    for (int off = 32; off > 0; off >>= 1) x += __shfl_xor(x, off, WAVE);
    return x;
}

// single-wavefront LDS ordering: LDS operations of one wave execute in order; this only stops the compiler from
// moving LDS accesses across it and drains lgkmcnt
__device__ __forceinline__ void wave_lds_sync()
{
    __builtin_amdgcn_fence(__ATOMIC_RELEASE, "workgroup");
    __builtin_amdgcn_wave_barrier();
    __builtin_amdgcn_fence(__ATOMIC_ACQUIRE, "workgroup");
}

// ---- the same pairing tree (lane l with l^32, l^16, l^8, l^4, l^2, l^1, in that order) on the VALU: no LDS crossbar ----
// A 64-bit value travels as its two dwords.  IEEE addition and fmax are commutative, so whichever lane of a pair holds which
// operand the pair ends with the same bits, exactly those of the butterfly above.  ALL 64 LANES MUST BE ACTIVE for the wave forms
// (quad_x1 / quad_x2 only need the lane's whole quad).
struct Dw2 { int lo, hi; };
__device__ __forceinline__ Dw2 dw2(double x) { return Dw2{__double2loint(x), __double2hiint(x)}; }
__device__ __forceinline__ Dw2 dw2(long long x) { return Dw2{(int)(unsigned long long)x, (int)((unsigned long long)x >> 32)}; }
__device__ __forceinline__ void from_dw2(Dw2 w, double &x) { x = __hiloint2double(w.hi, w.lo); }
__device__ __forceinline__ void from_dw2(Dw2 w, long long &x) { x = (long long)(((unsigned long long)(unsigned)w.hi << 32) | (unsigned)w.lo); }

// DPP move of every lane: CTRL 0x4E = quad_perm:[2,3,0,1] (l^2), 0xB1 = quad_perm:[1,0,3,2] (l^1), 0x128 = row_ror:8 (l^8)
template <int CTRL, class T>
__device__ __forceinline__ T dpp_all(T x)
{
    const Dw2 w = dw2(x);
    Dw2 r;
    // (every lane of these patterns has a source lane, so no lane keeps an old value: the form without one lets the move read
    //  its source where it is instead of a copy made for the purpose)
    r.lo = __builtin_amdgcn_mov_dpp(w.lo, CTRL, 0xf, 0xf, false);
    r.hi = __builtin_amdgcn_mov_dpp(w.hi, CTRL, 0xf, 0xf, false);
    T y; from_dw2(r, y); return y;
}
template <class T> __device__ __forceinline__ T quad_x1(T x) { return dpp_all<0xB1>(x); }
template <class T> __device__ __forceinline__ T quad_x2(T x) { return dpp_all<0x4E>(x); }
template <class T> __device__ __forceinline__ T row_x8(T x) { return dpp_all<0x128>(x); }
// l^4: row_ror:n hands lane i of a 16-lane row the value of lane (i - n) mod 16, so the lanes with bit 2 clear (banks 0 and 2,
// bank_mask 0x5) take row_ror:12 and the lanes with bit 2 set (banks 1 and 3, bank_mask 0xa) take row_ror:4
template <class T>
__device__ __forceinline__ T row_x4(T x)
{
    const Dw2 w = dw2(x);
    Dw2 r;
    r.lo = __builtin_amdgcn_mov_dpp(w.lo, 0x12C, 0xf, 0x5, false);       // (the other two banks are written by the second move)
    r.lo = __builtin_amdgcn_update_dpp(r.lo, w.lo, 0x124, 0xf, 0xa, false);
    r.hi = __builtin_amdgcn_mov_dpp(w.hi, 0x12C, 0xf, 0x5, false);
    r.hi = __builtin_amdgcn_update_dpp(r.hi, w.hi, 0x124, 0xf, 0xa, false);
    T y; from_dw2(r, y); return y;
}
// l^32 / l^16: v_permlane32_swap exchanges the upper half of its first operand with the lower half of its second (v_permlane16_swap:
// the odd rows of the first with the even rows of the second).  With the same value in both, every lane ends with its own value
// in one result and its partner's in the other; which is which depends on the half (row), and the commutative `op` need not know.
template <class T, class Op>
__device__ __forceinline__ T swap32_combine(T x, Op op)
{
    const Dw2 w = dw2(x);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)w.lo, (unsigned)w.lo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)w.hi, (unsigned)w.hi, false, false);
    T a, b;
    from_dw2(Dw2{(int)lo[0], (int)hi[0]}, a);
    from_dw2(Dw2{(int)lo[1], (int)hi[1]}, b);
    return op(a, b);
}
template <class T, class Op>
__device__ __forceinline__ T swap16_combine(T x, Op op)
{
    const Dw2 w = dw2(x);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)w.lo, (unsigned)w.lo, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)w.hi, (unsigned)w.hi, false, false);
    T a, b;
    from_dw2(Dw2{(int)lo[0], (int)hi[0]}, a);
    from_dw2(Dw2{(int)lo[1], (int)hi[1]}, b);
    return op(a, b);
}
struct OpAdd { template <class T> __device__ __forceinline__ T operator()(T a, T b) const { return a + b; } };
struct OpFmax { __device__ __forceinline__ double operator()(double a, double b) const { return fmax(a, b); } };
template <class T, class Op>
__device__ __forceinline__ T wave_reduce_dpp(T x, Op op)
{
    x = swap32_combine(x, op);
    x = swap16_combine(x, op);
    x = op(x, row_x8(x));
    x = op(x, row_x4(x));
    x = op(x, quad_x2(x));
    x = op(x, quad_x1(x));
    return x;
}
__device__ __forceinline__ double wave_sum_dpp(double x) { return wave_reduce_dpp(x, OpAdd()); }
__device__ __forceinline__ double wave_max_dpp(double x) { return wave_reduce_dpp(x, OpFmax()); }
__device__ __forceinline__ long long wave_sum_ll_dpp(long long x) { return wave_reduce_dpp(x, OpAdd()); }

// ---- several sums at once: the first two levels transpose them ----
// v_permlane32_swap on two DIFFERENT registers a, b leaves a = [a's lower half | b's lower half] and b = [a's upper half | b's
// upper half], so their sum holds a[l] + a[l^32] in lanes 0..31 and b[l] + b[l^32] in lanes 32..63: level 32 of two butterflies
// for one swap per dword and one addition.  v_permlane16_swap does the same with the rows: the sum holds a's pairs (l, l^16) in
// the even rows and b's in the odd rows.  The pairs and the order of the levels are those of wave_sum_dpp, and an addition does
// not care which lane holds which operand, so every total keeps its bits; it ends in one group of lanes instead of all 64.
__device__ __forceinline__ double swap32_add2(double a, double b)
{
    const Dw2 wa = dw2(a), wb = dw2(b);
    const auto lo = __builtin_amdgcn_permlane32_swap((unsigned)wa.lo, (unsigned)wb.lo, false, false);
    const auto hi = __builtin_amdgcn_permlane32_swap((unsigned)wa.hi, (unsigned)wb.hi, false, false);
    double x, y;
    from_dw2(Dw2{(int)lo[0], (int)hi[0]}, x);
    from_dw2(Dw2{(int)lo[1], (int)hi[1]}, y);
    return x + y;
}
__device__ __forceinline__ double swap16_add2(double a, double b)
{
    const Dw2 wa = dw2(a), wb = dw2(b);
    const auto lo = __builtin_amdgcn_permlane16_swap((unsigned)wa.lo, (unsigned)wb.lo, false, false);
    const auto hi = __builtin_amdgcn_permlane16_swap((unsigned)wa.hi, (unsigned)wb.hi, false, false);
    double x, y;
    from_dw2(Dw2{(int)lo[0], (int)hi[0]}, x);
    from_dw2(Dw2{(int)lo[1], (int)hi[1]}, y);
    return x + y;
}
// wave_sum_multi<OB>(s, t), OB = 2, 4 or 8, ALL 64 LANES ACTIVE: the OB wave sums of s[0..OB) in wave_sum_multi_regs(OB) registers.
//   OB = 2: t[0] holds the total of s[0] in lanes 0..31 and of s[1] in lanes 32..63;
//   OB = 4, 8: row r (lanes 16r..16r+15) of t[j] holds the total of s[4j + 2(r & 1) + (r >> 1)]
// (wave_sum_multi_index); wave_sum_multi_owner picks one lane of each group, the one that stores the total.
__host__ __device__ constexpr int wave_sum_multi_regs(int OB) { return OB <= 4 ? 1 : OB / 4; }
template <int OB> __device__ __forceinline__ uint32_t wave_sum_multi_index(uint32_t lane, int j)
{
    const uint32_t row = lane >> 4;
    return OB == 2 ? row >> 1 : 4u * j + (((row & 1u) << 1) | (row >> 1));
}
template <int OB> __device__ __forceinline__ bool wave_sum_multi_owner(uint32_t lane) { return (lane & (OB == 2 ? 31u : 15u)) == 0; }
template <int OB>
__device__ __forceinline__ void wave_sum_multi(const double (&s)[OB], double (&t)[wave_sum_multi_regs(OB)])
{
    static_assert(OB == 2 || OB == 4 || OB == 8, "pairs of pairs");
    constexpr int NR = wave_sum_multi_regs(OB);
    double h[OB / 2];
#pragma unroll
    for (int j = 0; j < OB / 2; j++) h[j] = swap32_add2(s[2 * j], s[2 * j + 1]);
    if constexpr (OB == 2) t[0] = swap16_combine(h[0], OpAdd());
    else {
#pragma unroll
        for (int j = 0; j < NR; j++) t[j] = swap16_add2(h[2 * j], h[2 * j + 1]);
    }
#pragma unroll
    for (int j = 0; j < NR; j++) t[j] += row_x8(t[j]);
#pragma unroll
    for (int j = 0; j < NR; j++) t[j] += row_x4(t[j]);
#pragma unroll
    for (int j = 0; j < NR; j++) t[j] += quad_x2(t[j]);
#pragma unroll
    for (int j = 0; j < NR; j++) t[j] += quad_x1(t[j]);
}

// A kernel argument the entry block must already hold in scalar registers.  The compiler otherwise sinks each argument's scalar
// load to the block of its first use, behind every early-out branch: one dependent round trip to the kernarg segment per group of
// arguments before the first useful load.  Named here together, the arguments arrive in one batch behind one wait.
// (This steers the compiler, it is not a guarantee: profiles/r06_isa_counts.txt records the entry blocks it gave; no test holds them.)
template <class T> __device__ __forceinline__ void kernarg_now(const T &x) { asm volatile("" ::"s"(x)); }
template <class T, class... R> __device__ __forceinline__ void kernarg_now(const T &x, const R &...rest) { kernarg_now(x); kernarg_now(rest...); }
// A wave-uniform word nobody writes while this kernel runs, read with a scalar load.  (The compiler takes a volatile statement
// such as kernarg_now for a store to anything, and a plain load behind one becomes a vector load with a vector wait.)
__device__ __forceinline__ int32_t uniform_word(const int32_t *p) { return *(const __attribute__((address_space(4))) int32_t *)p; }
// a lane value the optimiser must take as it is HERE: keeps a load's first use (and its wait) where the code puts it
template <class T> __device__ __forceinline__ T lane_value_here(T x) { asm volatile("" : "+v"(x)); return x; }
// the same for a wave-uniform value in a scalar register: what is computed from it stays behind this point (a rarely taken
// branch keeps its own comparisons instead of having them hoisted, and their results spilled, in front of the common path)
template <class T> __device__ __forceinline__ T uniform_value_here(T x) { asm volatile("" : "+s"(x)); return x; }

// wave_probe.hip -- bluest_wave_reduce_probe (include/bluest_hip.h): what every lane holds after the DPP / permlane reductions of
// common.hpp, for tests/test_gpu_wave_reduce.py, and bluest_wave_reduce_multi_probe: the totals of wave_sum_multi as the lanes that
// own them store them, for tests/test_gpu_wave_reduce_multi.py.  One wavefront per workgroup, all 64 lanes active.
#include "common.hpp"

__global__ __launch_bounds__(64) void k_wave_reduce_probe(const double *__restrict__ in, double *__restrict__ sum_out, double *__restrict__ max_out,
                                                         double *__restrict__ quad_out, long long *__restrict__ isum_out)
{
    const int64_t i = (int64_t)blockIdx.x * 64 + threadIdx.x;
    const double x = in[i];
    sum_out[i] = wave_sum_dpp(x);
    max_out[i] = wave_max_dpp(x);
    double q = x;
    q += quad_x1(q);
    q += quad_x2(q);
    quad_out[i] = q;
    isum_out[i] = wave_sum_ll_dpp(__double_as_longlong(x) >> 8);
}

extern "C" int bluest_wave_reduce_probe(const double *in_dev, int64_t n_rows, double *sum_dev, double *max_dev, double *quad_dev,
                                        int64_t *isum_dev, void *stream)
{
    int rc = require_gpu(); if (rc) return rc;
    if (!in_dev || !sum_dev || !max_dev || !quad_dev || !isum_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (n_rows < 1 || n_rows > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "n_rows out of range");
    hipLaunchKernelGGL(k_wave_reduce_probe, dim3((unsigned)n_rows), dim3(64), 0, (hipStream_t)stream, in_dev, sum_dev, max_dev, quad_dev,
                       reinterpret_cast<long long *>(isum_dev));
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

// row b: OB vectors of 64 doubles in, OB totals out, each written by the lane k_phi_chunks_shared<OB> stores it from
template <int OB>
__global__ __launch_bounds__(64) void k_wave_reduce_multi_probe(const double *__restrict__ in, double *__restrict__ out)
{
    constexpr int NR = wave_sum_multi_regs(OB);
    const uint32_t lane = threadIdx.x;
    double s[OB], t[NR];
#pragma unroll
    for (int oo = 0; oo < OB; oo++) s[oo] = in[((int64_t)blockIdx.x * OB + oo) * 64 + lane];
    wave_sum_multi<OB>(s, t);
#pragma unroll
    for (int j = 0; j < NR; j++)
        if (wave_sum_multi_owner<OB>(lane)) out[(int64_t)blockIdx.x * OB + wave_sum_multi_index<OB>(lane, j)] = t[j];
}

extern "C" int bluest_wave_reduce_multi_probe(const double *in_dev, int64_t n_rows, int ob, double *out_dev, void *stream)
{
    int rc = require_gpu(); if (rc) return rc;
    if (!in_dev || !out_dev) return fail(BLUEST_ERR_ARG, "null pointer");
    if (n_rows < 1 || n_rows > 0x7fffffffLL) return fail(BLUEST_ERR_ARG, "n_rows out of range");
    const dim3 grid((unsigned)n_rows);
    hipStream_t st = (hipStream_t)stream;
    switch (ob) {
    case 2: hipLaunchKernelGGL(k_wave_reduce_multi_probe<2>, grid, dim3(64), 0, st, in_dev, out_dev); break;
    case 4: hipLaunchKernelGGL(k_wave_reduce_multi_probe<4>, grid, dim3(64), 0, st, in_dev, out_dev); break;
    case 8: hipLaunchKernelGGL(k_wave_reduce_multi_probe<8>, grid, dim3(64), 0, st, in_dev, out_dev); break;
    default: return fail(BLUEST_ERR_ARG, "ob=%d: 2, 4 or 8", ob);
    }
    HIP_TRY(hipGetLastError());
    return BLUEST_OK;
}

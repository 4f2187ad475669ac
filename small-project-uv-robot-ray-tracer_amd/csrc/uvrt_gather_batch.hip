// uvrt_gather_batch.hip -- the batched direct gather (include/uvrt.h "batched direct gather"): the
// generate and reduce kernels of uvrt_gather_direct_batch.
//
// A batch is `count` gather launches over one triangle range and one sample count S.  Its unit of work is a pair
// q = k * tri_count + lt (launch k, triangle first_tri + lt), launch-major so that the rays of one lamp stay together; pairs go
// through lane 0's ray buffers in chunks of floor(capacity / S), and a chunk may straddle a launch boundary.  Per chunk
// k_gather_generate_batch<MODE> makes the S samples of every pair with the rule of k_gather_generate<MODE> (the shared
// gather_sample of uvrt_gather_sample.h), reading the pair's lamp from a device table -- the launch index differs from lane to
// lane, so it cannot index a kernel argument --, k_occlude_free (uvrt_occlude.hip) answers them and k_gather_reduce_batch /
// k_gather_reduce_var_batch<MODE> sum every pair's samples in sample order into plane k of E_b (and V_b) with the shared sums of
// k_gather_reduce / k_gather_reduce_var<MODE>.  No atomics: plane k is a pure function of launch k's arguments, bit for bit what
// uvrt_gather_direct leaves in `expected` (`variance`).  This file is built without contraction, every operator is one rounding.
#include "uvrt_gather_sample.h"

namespace uvrt {

// pair p of the chunk: its launch and its triangle's offset into the range
__device__ __forceinline__ void batch_pair(const GatherBatchParams& g, uint32_t p, uint32_t& k, uint32_t& lt)
{
    const uint32_t x = (uint32_t)g.lt0 + p;
    const uint32_t dk = x / (uint32_t)g.tri_count;
    k = (uint32_t)g.k0 + dk;
    lt = x - dk * (uint32_t)g.tri_count;
}

template <int MODE>
__global__ __launch_bounds__(256) void k_gather_generate_batch(GatherBatchParams g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.pair_count * g.samples) return;
    const uint32_t p = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)p * g.samples);
    uint32_t k, lt;
    batch_pair(g, p, k, lt);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const GatherBatchLaunch b = g.table[k];
    const GatherLamp l = {b.fx, b.fy, b.fz, b.tx, b.ty, b.tz, b.light_length, b.seed, b.seed_hash};
    const GatherSample o = gather_sample<MODE>(g.gtris, l, t, s, g.samples);
    g.rays[i] = o.ray;
    g.oxz[i] = o.oxz;
    g.tmax[i] = o.tmax;
    g.w[i] = o.w;
}

void launch_gather_generate_batch(const GatherBatchParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.pair_count * p.samples;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.mode == 1) hipLaunchKernelGGL((k_gather_generate_batch<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gather_generate_batch<0>), grid, dim3(256), 0, s, p);
}

// one thread per pair of the chunk
__global__ __launch_bounds__(256) void k_gather_reduce_batch(GatherBatchParams g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.pair_count) return;
    uint32_t k, lt;
    batch_pair(g, (uint32_t)i, k, lt);
    const size_t t = (size_t)g.first_tri + (size_t)lt;
    const double nn = gather_tri_nn(g.gtris, t);
    const size_t at = (size_t)i * (size_t)g.samples;
    g.e_planes[(size_t)k * (size_t)g.T + t] =
        gather_expected(nn, gather_sum(g.w, g.occluded, at, g.samples), g.samples, g.table[k].photons_equiv);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_gather_reduce_var_batch(GatherBatchParams g)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= g.pair_count) return;
    uint32_t k, lt;
    batch_pair(g, (uint32_t)i, k, lt);
    const size_t t = (size_t)g.first_tri + (size_t)lt;
    const double nn = gather_tri_nn(g.gtris, t);
    const size_t at = (size_t)i * (size_t)g.samples;
    const size_t o = (size_t)k * (size_t)g.T + t;
    gather_expected_var<MODE>(g.w, g.occluded, at, g.samples, nn, gather_sum(g.w, g.occluded, at, g.samples),
                              g.table[k].photons_equiv, g.e_planes[o], g.v_planes[o]);
}

void launch_gather_reduce_batch(const GatherBatchParams& p, bool variance, hipStream_t s)
{
    if (p.pair_count <= 0) return;
    const dim3 grid((unsigned)((p.pair_count + 255) / 256));
    if (!variance) hipLaunchKernelGGL(k_gather_reduce_batch, grid, dim3(256), 0, s, p);
    else if (p.mode == 1) hipLaunchKernelGGL((k_gather_reduce_var_batch<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gather_reduce_var_batch<0>), grid, dim3(256), 0, s, p);
}

}  // namespace uvrt

// uvrt_links.hip -- recorded hit links and the multi-bounce gather over them (include/uvrt.h "recorded hit links",
// DESIGN.md section 18).
//
// The rays of the one-bounce gather (uvrt_indirect.hip) depend on the scene, S2 and the seed alone; only the source values
// looked up at their hits change from launch to launch.  k_links_store keeps, for every (triangle, sample), the triangle
// the ray sees or -1 -- with the filter of k_indirect_reduce's y_s baked in -- and k_links_apply turns one bounce into a
// lookup-and-sum: no generate kernel, no traversal.  Bounce b + 1 is the same kernel over bounce b's irradiance plane.
//
// Layout: links[s * T + t], sample-major, so a wave's 64 triangles read 256 contiguous bytes per sample.  The irradiance
// e[h] = source[h] / (0.5 * nn_h) is a function of h alone, so it is computed once per bounce into an f64[T] plane (it stays
// in every XCD's L2) instead of once per sample: the same bits, no division and no normal in the sum.
// One thread per triangle walks its S2 links in sample order: the contract fixes the order of the sum.  The loads of a
// group of samples are issued together, only the adds are chained.  One plain launch per bounce; every loop is bounded by
// S2.  No atomics.  Only + - * / sqrt: this file is built without contraction, every operator below is one rounding.
#include "uvrt_device.h"

namespace uvrt {

// |cross(e1, e2)| in f64, where the normal itself is not asked for
__device__ __forceinline__ double tri_normal_len(const float4 e1, const float4 e2)
{
    double nx, ny, nz;
    return tri_normal(e1, e2, nx, ny, nz);
}

// thread i = (sample s, local triangle lt), lt fastest: the stores are contiguous, the 8-byte reads S2 * 8 bytes apart
__global__ __launch_bounds__(256) void k_links_store(LinksStoreParams p)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.tri_count * p.samples) return;
    const uint32_t s = (uint32_t)i / (uint32_t)p.tri_count, lt = (uint32_t)i - s * (uint32_t)p.tri_count;    // (T * S2 < 2^31)
    const uint32_t t = (uint32_t)p.first_tri + lt;
    const uint32_t h = p.hit[(size_t)lt * (size_t)p.samples + s].y;
    int32_t link = -1;
    if (h < (uint32_t)p.T && h != t) {                  // (0xFFFFFFFF, a miss, is no triangle's id)
        const double nh = tri_normal_len(p.gtris[(size_t)h * 3 + 1], p.gtris[(size_t)h * 3 + 2]);
        if (nh > 0.0) link = (int32_t)h;
    }
    p.links[(size_t)s * (size_t)p.T + t] = link;
}

void launch_links_store(const LinksStoreParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_links_store, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_links_irradiance(const float4* __restrict__ gtris, const double* __restrict__ source,
                                                          double* __restrict__ e, int32_t T)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= T) return;
    const double nh = tri_normal_len(gtris[(size_t)h * 3 + 1], gtris[(size_t)h * 3 + 2]);
    e[h] = nh > 0.0 ? source[h] / (0.5 * nh) : 0.0;
}

void launch_links_irradiance(const float4* gtris, const double* source, double* e, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_links_irradiance, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, gtris, source, e, T);
}

// the irradiance a link points at; -1 reads entry 0 and drops it, so the load needs no branch
__device__ __forceinline__ double linked_value(const double* __restrict__ e, int32_t link)
{
    const double v = e[link < 0 ? 0 : link];
    return link < 0 ? 0.0 : v;
}

// 64 threads per workgroup: T triangles are fewer waves than the chip has SIMDs, so every wave gets a CU slot of its own
constexpr int LINKS_APPLY_BLOCK = 64;
constexpr int LINKS_UNROLL = 8;

__global__ __launch_bounds__(LINKS_APPLY_BLOCK) void k_links_apply(LinksApplyParams p)
{
    const int i = blockIdx.x * LINKS_APPLY_BLOCK + threadIdx.x;
    if (i >= p.tri_count) return;
    const size_t t = (size_t)p.first_tri + (size_t)i;
    const size_t T = (size_t)p.T;
    const double nn = tri_normal_len(p.gtris[t * 3 + 1], p.gtris[t * 3 + 2]);
    const int32_t* __restrict__ lp = p.links + t;
    const double* __restrict__ e = p.e_in;
    double sum = 0.0;
    int32_t s = 0;
    for (; s + LINKS_UNROLL <= p.samples; s += LINKS_UNROLL) {
        int32_t l[LINKS_UNROLL];
        double v[LINKS_UNROLL];
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) l[u] = lp[(size_t)(s + u) * T];
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) v[u] = linked_value(e, l[u]);
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) sum = sum + v[u];
    }
    for (; s < p.samples; ++s) sum = sum + linked_value(e, lp[(size_t)s * T]);
    const double g = nn == 0.0 ? 0.0 : ((double)p.reflectance * (0.5 * nn)) * ((2.0 * sum) / (double)p.samples);
    if (p.e_out) p.e_out[t] = nn > 0.0 ? g / (0.5 * nn) : 0.0;
    const double total = p.total_in ? p.total_in[t] + g : g;
    if (p.total_out) p.total_out[t] = total;
    if (p.expected) p.expected[t] = p.add ? p.expected[t] + total : total;
}

void launch_links_apply(const LinksApplyParams& p, hipStream_t s)
{
    if (p.tri_count <= 0) return;
    hipLaunchKernelGGL(k_links_apply, dim3((unsigned)((p.tri_count + LINKS_APPLY_BLOCK - 1) / LINKS_APPLY_BLOCK)),
                       dim3(LINKS_APPLY_BLOCK), 0, s, p);
}

// Test hook: thread i = (local triangle, sample), sample fastest: the triangle-major order of uvrt_read_indirect_links
__global__ __launch_bounds__(256) void k_links_export(const int32_t* __restrict__ links, int32_t* __restrict__ out, int32_t first_tri,
                                                      int32_t tri_count, int32_t samples, int32_t T)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)tri_count * samples) return;
    const uint32_t lt = (uint32_t)i / (uint32_t)samples, s = (uint32_t)i - lt * (uint32_t)samples;            // (T * S2 < 2^31)
    out[i] = links[(size_t)s * (size_t)T + (size_t)first_tri + lt];
}

void launch_links_export(const int32_t* links, int32_t* out, int32_t first_tri, int32_t tri_count, int32_t samples, int32_t T,
                         hipStream_t s)
{
    const int64_t n = (int64_t)tri_count * samples;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_links_export, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, links, out, first_tri, tri_count, samples, T);
}

}  // namespace uvrt

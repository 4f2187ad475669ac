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
// The sided forms at the end of the file (include/uvrt.h "face-resolved gather and bounces") keep the face
// of the hit triangle a ray arrives on in bit 0 of the link and one irradiance per face, interleaved e[2 * h + face]: the same
// layout, loads and launch structure, two sums per triangle.
// The mapped forms behind them (include/uvrt.h "per-face reflectance") give every face a reflectance of
// its own: the planes of the bounces then hold radiosities rho[f][h] * e[f][h], multiplied in where a plane is written.
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

// ---- the sided forms: every triangle an opaque sheet whose two faces keep their own irradiance ----

// k_links_store with the arrival face in bit 0: a = 0 when the ray meets the side n_h points to (n_h . dir < 0).  dir is the
// f32 direction k_indirect_generate wrote into the chunk's rays; the closest-hit kernel reads them only.
__global__ __launch_bounds__(256) void k_links_store_sided(LinksStoreParams p, const float4* __restrict__ rays)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)p.tri_count * p.samples) return;
    const uint32_t s = (uint32_t)i / (uint32_t)p.tri_count, lt = (uint32_t)i - s * (uint32_t)p.tri_count;    // (T * S2 < 2^31)
    const uint32_t t = (uint32_t)p.first_tri + lt;
    const size_t r = (size_t)lt * (size_t)p.samples + s;
    const uint32_t h = p.hit[r].y;
    int32_t link = -1;
    if (h < (uint32_t)p.T && h != t) {
        double nx, ny, nz;
        const double nh = tri_normal(p.gtris[(size_t)h * 3 + 1], p.gtris[(size_t)h * 3 + 2], nx, ny, nz);
        const float4 d = rays[r];
        const double c = (nx * (double)d.x + ny * (double)d.y) + nz * (double)d.z;
        if (nh > 0.0) link = (int32_t)((h << 1) | (c < 0.0 ? 0u : 1u));          // (S2 >= 2: h < T < 2^30)
    }
    p.links[(size_t)s * (size_t)p.T + t] = link;
}

void launch_links_store_sided(const LinksStoreParams& p, const float4* rays, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_links_store_sided, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p, rays);
}

__global__ __launch_bounds__(256) void k_links_irradiance_sided(const float4* __restrict__ gtris, const double* __restrict__ faces,
                                                                double* __restrict__ e, int32_t T)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= T) return;
    const double nh = tri_normal_len(gtris[(size_t)h * 3 + 1], gtris[(size_t)h * 3 + 2]);
    e[(size_t)h * 2 + 0] = nh > 0.0 ? faces[h] / (0.5 * nh) : 0.0;
    e[(size_t)h * 2 + 1] = nh > 0.0 ? faces[(size_t)T + h] / (0.5 * nh) : 0.0;
}

void launch_links_irradiance_sided(const float4* gtris, const double* faces, double* e, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_links_irradiance_sided, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, gtris, faces, e, T);
}

// One thread per triangle, one accumulator per face: sample s leaves face s & 1, so the even slots of a group of the unroll
// go to face 0 and the odd ones to face 1 (LINKS_UNROLL is even and s starts at 0).  The loads of a group are issued together
// as in k_links_apply; the two chains of adds are independent, each half as long as k_links_apply's one.  A sided link is the
// index into the interleaved plane, so linked_value is the plain kernel's load.
__global__ __launch_bounds__(LINKS_APPLY_BLOCK) void k_links_apply_sided(LinksApplyParams p)
{
    static_assert(LINKS_UNROLL % 2 == 0, "a group of the unroll holds whole (face 0, face 1) pairs");
    const int i = blockIdx.x * LINKS_APPLY_BLOCK + threadIdx.x;
    if (i >= p.tri_count) return;
    const size_t t = (size_t)p.first_tri + (size_t)i;
    const size_t T = (size_t)p.T;
    const double nn = tri_normal_len(p.gtris[t * 3 + 1], p.gtris[t * 3 + 2]);
    const int32_t* __restrict__ lp = p.links + t;
    const double* __restrict__ e = p.e_in;
    double sum0 = 0.0, sum1 = 0.0;
    int32_t s = 0;
    for (; s + LINKS_UNROLL <= p.samples; s += LINKS_UNROLL) {
        int32_t l[LINKS_UNROLL];
        double v[LINKS_UNROLL];
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) l[u] = lp[(size_t)(s + u) * T];
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) v[u] = linked_value(e, l[u]);
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; u += 2) {
            sum0 = sum0 + v[u];
            sum1 = sum1 + v[u + 1];
        }
    }
    for (; s + 2 <= p.samples; s += 2) {            // (samples is even)
        const int32_t l0 = lp[(size_t)s * T], l1 = lp[(size_t)(s + 1) * T];
        const double v0 = linked_value(e, l0), v1 = linked_value(e, l1);
        sum0 = sum0 + v0;
        sum1 = sum1 + v1;
    }
    const double k = (double)p.reflectance * (0.5 * nn);
    const double g0 = nn == 0.0 ? 0.0 : k * ((2.0 * sum0) / (double)p.samples);
    const double g1 = nn == 0.0 ? 0.0 : k * ((2.0 * sum1) / (double)p.samples);
    if (p.e_out) {
        p.e_out[t * 2 + 0] = nn > 0.0 ? g0 / (0.5 * nn) : 0.0;
        p.e_out[t * 2 + 1] = nn > 0.0 ? g1 / (0.5 * nn) : 0.0;
    }
    const double g = g0 + g1;
    const double total = p.total_in ? p.total_in[t] + g : g;
    if (p.total_out) p.total_out[t] = total;
    if (p.expected) p.expected[t] = p.add ? p.expected[t] + total : total;
}

void launch_links_apply_sided(const LinksApplyParams& p, hipStream_t s)
{
    if (p.tri_count <= 0) return;
    hipLaunchKernelGGL(k_links_apply_sided, dim3((unsigned)((p.tri_count + LINKS_APPLY_BLOCK - 1) / LINKS_APPLY_BLOCK)),
                       dim3(LINKS_APPLY_BLOCK), 0, s, p);
}

// ---- the mapped forms: the sided bounce with a reflectance per face, rho[f * T + t] f32[2][T] ----
// The reflectance belongs to the face that emits, so it is multiplied into the plane the links point at -- the radiosity
// r[2 * h + f] = rho[f][h] * e[f][h] -- and the receiver's epilogue carries none.  The plane keeps the interleaved layout: a
// sided link is still the index of what it points at and linked_value is still the load.

__global__ __launch_bounds__(256) void k_links_radiosity_sided(const float4* __restrict__ gtris, const double* __restrict__ faces,
                                                               const float* __restrict__ rho, double* __restrict__ r, int32_t T)
{
    const int h = blockIdx.x * 256 + threadIdx.x;
    if (h >= T) return;
    const double nh = tri_normal_len(gtris[(size_t)h * 3 + 1], gtris[(size_t)h * 3 + 2]);
    r[(size_t)h * 2 + 0] = nh > 0.0 ? (double)rho[h] * (faces[h] / (0.5 * nh)) : 0.0;
    r[(size_t)h * 2 + 1] = nh > 0.0 ? (double)rho[(size_t)T + h] * (faces[(size_t)T + h] / (0.5 * nh)) : 0.0;
}

void launch_links_radiosity_sided(const float4* gtris, const double* faces, const float* rho, double* r, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_links_radiosity_sided, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, gtris, faces, rho, r, T);
}

// k_links_apply_sided's loop, a copy of it (a shared helper would have to leave that kernel's code as it is, instruction for
// instruction); the epilogue has no reflectance on the receiver and writes the next bounce's radiosity, rho of this triangle's
// own faces times the irradiance they have just received: two coalesced f32 loads per thread, no second launch per bounce.
__global__ __launch_bounds__(LINKS_APPLY_BLOCK) void k_links_apply_mapped(LinksMappedParams p)
{
    static_assert(LINKS_UNROLL % 2 == 0, "a group of the unroll holds whole (face 0, face 1) pairs");
    const int i = blockIdx.x * LINKS_APPLY_BLOCK + threadIdx.x;
    if (i >= p.tri_count) return;
    const size_t t = (size_t)p.first_tri + (size_t)i;
    const size_t T = (size_t)p.T;
    const double nn = tri_normal_len(p.gtris[t * 3 + 1], p.gtris[t * 3 + 2]);
    const int32_t* __restrict__ lp = p.links + t;
    const double* __restrict__ r = p.r_in;
    double sum0 = 0.0, sum1 = 0.0;
    int32_t s = 0;
    for (; s + LINKS_UNROLL <= p.samples; s += LINKS_UNROLL) {
        int32_t l[LINKS_UNROLL];
        double v[LINKS_UNROLL];
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) l[u] = lp[(size_t)(s + u) * T];
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; ++u) v[u] = linked_value(r, l[u]);
#pragma unroll
        for (int u = 0; u < LINKS_UNROLL; u += 2) {
            sum0 = sum0 + v[u];
            sum1 = sum1 + v[u + 1];
        }
    }
    for (; s + 2 <= p.samples; s += 2) {            // (samples is even)
        const int32_t l0 = lp[(size_t)s * T], l1 = lp[(size_t)(s + 1) * T];
        const double v0 = linked_value(r, l0), v1 = linked_value(r, l1);
        sum0 = sum0 + v0;
        sum1 = sum1 + v1;
    }
    const double g0 = nn == 0.0 ? 0.0 : (0.5 * nn) * ((2.0 * sum0) / (double)p.samples);
    const double g1 = nn == 0.0 ? 0.0 : (0.5 * nn) * ((2.0 * sum1) / (double)p.samples);
    if (p.r_out) {
        const double rho0 = (double)p.rho[t], rho1 = (double)p.rho[T + t];
        p.r_out[t * 2 + 0] = nn > 0.0 ? rho0 * (g0 / (0.5 * nn)) : 0.0;
        p.r_out[t * 2 + 1] = nn > 0.0 ? rho1 * (g1 / (0.5 * nn)) : 0.0;
    }
    const double g = g0 + g1;
    const double total = p.total_in ? p.total_in[t] + g : g;
    if (p.total_out) p.total_out[t] = total;
    if (p.expected) p.expected[t] = p.add ? p.expected[t] + total : total;
}

void launch_links_apply_mapped(const LinksMappedParams& p, hipStream_t s)
{
    if (p.tri_count <= 0) return;
    hipLaunchKernelGGL(k_links_apply_mapped, dim3((unsigned)((p.tri_count + LINKS_APPLY_BLOCK - 1) / LINKS_APPLY_BLOCK)),
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

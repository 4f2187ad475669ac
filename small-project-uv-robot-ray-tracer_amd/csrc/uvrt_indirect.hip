// uvrt_indirect.hip -- the closest-hit query that deposits nothing, and the one-bounce final gather built on it
// (include/uvrt.h "one diffuse bounce").
//
// k_closest_free is uvrt_query.h's traversal without FIRST_HIT -- a lane runs to the end of its stack, so dist / triID end as
// extend.cl leaves them for a ray whose dist is preset to tmax -- and an answer of one record per ray slot,
// hit[slot] = (dist bits, dist bits == tmax bits ? 0xFFFFFFFF : triID).  Beyond the traversal the disc rejection below is
// bounded by 8 rounds, the reduction by S2.
//
// The bounce: k_indirect_generate makes, for every (triangle, sample), a point on the triangle and a cosine-distributed
// direction about its normal (even samples leave one face, odd samples the other); k_closest_free finds what each ray sees;
// k_indirect_reduce looks up the source plane at the hit triangles and sums per triangle in sample order.  No atomics: the
// plane is a pure function of the arguments.  Only + - * / sqrt: this file is built without contraction, every operator
// below is one rounding.
#include "uvrt_query.h"

namespace uvrt {

// the answer of the ray a lane has finished
struct ClosestAnswer {
    const ClosestParams& cp;
    __device__ __forceinline__ void operator()(const LaneF& L, float tmax, uint32_t slot) const
    {
        if (slot != NO_SLOT) {
            const uint32_t d = __float_as_uint(L.po.y);
            cp.hit[slot] = make_uint2(d, d == __float_as_uint(tmax) ? NO_TRI : L.triID);
        }
    }
};

template <int FL>
__global__ __launch_bounds__(256, FREE_GRID_PER_CU) void k_closest_free(ClosestParams cp)
{
    run_query_rays<FL, false>(cp.e, cp.oxz, cp.tmax, ClosestAnswer{cp});
}

bool launch_closest_free(const ClosestParams& p, int grid_per_cu, hipStream_t s)
{
    return launch_query_free(p, k_closest_free<0>, k_closest_free<1>, grid_per_cu, s);
}

// ---- the one-bounce gather ----

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(256) void k_indirect_generate(IndirectGenParams g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.tri_count * g.samples) return;
    const uint32_t lt = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lt * g.samples);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const uint32_t j = t * (uint32_t)g.samples + s;
    uint32_t rng = wang_hash(j ^ g.seed_hash);
    float a = random_float(rng);
    float b = random_float(rng);
    if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
    const float4 v0 = g.gtris[(size_t)t * 3 + 0], e1 = g.gtris[(size_t)t * 3 + 1], e2 = g.gtris[(size_t)t * 3 + 2];
    const float px = (v0.x + a * e1.x) + b * e2.x;
    const float py = (v0.y + a * e1.y) + b * e2.y;
    const float pz = (v0.z + a * e1.z) + b * e2.z;
    // generate.cl:25-28's point in the unit disc, bounded: after 8 rejected rounds the centre
    double x = 0.0, y = 0.0;
    for (int round = 0; round < 8; ++round) {
        const float xf = random_float(rng);
        const float yf = random_float(rng);
        const double xd = (double)(xf * 2.0f - 1.0f), yd = (double)(yf * 2.0f - 1.0f);
        if (xd * xd + yd * yd <= 1.0) { x = xd; y = yd; break; }
    }
    double nx, ny, nz;
    const double nn = tri_normal(e1, e2, nx, ny, nz);
    const double Ex = (double)e1.x, Ey = (double)e1.y, Ez = (double)e1.z;
    const double l1 = sqrt((Ex * Ex + Ey * Ey) + Ez * Ez);
    const double Tx = Ex / l1, Ty = Ey / l1, Tz = Ez / l1;
    const double Bx = (ny * Tz - nz * Ty) / nn, By = (nz * Tx - nx * Tz) / nn, Bz = (nx * Ty - ny * Tx) / nn;
    const double z = sqrt(1.0 - (x * x + y * y));
    const double zz = ((s & 1u) ? -z : z) / nn;
    const float dx = (float)(((x * Tx) + (y * Bx)) + (zz * nx));
    const float dy = (float)(((x * Ty) + (y * By)) + (zz * ny));
    const float dz = (float)(((x * Tz) + (y * Bz)) + (zz * nz));
    float4 ray = make_float4(dx, dy, dz, py);
    float tm = 1e30f;
    if (nn == 0.0 || !finite_f32(dx) || !finite_f32(dy) || !finite_f32(dz) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        ray = make_float4(0.f, 1.f, 0.f, py);       // not traced: tmax 0 accepts no hit
        tm = 0.0f;
    }
    g.rays[i] = ray;
    g.oxz[i] = make_float2(px, pz);
    g.tmax[i] = tm;
}

void launch_indirect_generate(const IndirectGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_indirect_generate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_indirect_reduce(IndirectReduceParams r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.tri_count) return;
    const size_t t = (size_t)r.first_tri + (size_t)i;
    double nx, ny, nz;
    const double nn = tri_normal(r.gtris[t * 3 + 1], r.gtris[t * 3 + 2], nx, ny, nz);
    double sum = 0.0;
    const size_t at = (size_t)i * (size_t)r.samples;
    for (int32_t s = 0; s < r.samples; ++s) {
        const uint32_t h = r.hit[at + s].y;
        double ys = 0.0;
        if (h < (uint32_t)r.T && h != (uint32_t)t) {        // (NO_TRI, a miss, is no triangle's id)
            const double nh = tri_normal(r.gtris[(size_t)h * 3 + 1], r.gtris[(size_t)h * 3 + 2], nx, ny, nz);
            if (nh > 0.0) ys = r.source[h] / (0.5 * nh);
        }
        sum = sum + ys;
    }
    const double ind = nn == 0.0 ? 0.0 : ((double)r.reflectance * (0.5 * nn)) * ((2.0 * sum) / (double)r.samples);
    r.expected[t] = r.add ? r.expected[t] + ind : ind;
}

void launch_indirect_reduce(const IndirectReduceParams& p, hipStream_t s)
{
    if (p.tri_count <= 0) return;
    hipLaunchKernelGGL(k_indirect_reduce, dim3((unsigned)((p.tri_count + 255) / 256)), dim3(256), 0, s, p);
}

// Test hook: the rays of a chunk as the reference's 32-byte Ray records, dist = tmax
__global__ __launch_bounds__(256) void k_export_closest_rays(const float4* __restrict__ rays, const float2* __restrict__ oxz,
                                                             const float* __restrict__ tmax, float4* __restrict__ out, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float4 rec = rays[i];
    const float2 o = oxz[i];
    out[i * 2 + 0] = make_float4(rec.x, rec.y, rec.z, o.x);
    out[i * 2 + 1] = make_float4(rec.w, o.y, tmax[i], 0.f);
}

void launch_export_closest_rays(const float4* rays, const float2* oxz, const float* tmax, void* out32, int64_t count, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_export_closest_rays, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, rays, oxz, tmax,
                       (float4*)out32, count);
}

}  // namespace uvrt

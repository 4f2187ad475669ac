// uvrt_occlude.hip -- shadow rays (an occlusion query: a ray with a maximum distance that stops at its first hit) and the
// per-triangle direct gather built on them (include/uvrt.h "shadow rays and the direct gather").
//
// k_occlude_free is uvrt_query.h's traversal with FIRST_HIT -- after every step a lane whose dist bits differ from its tmax
// bits is finished: some triangle was accepted, which is all the query asks -- and an answer of one byte per ray slot,
// occluded[slot] = dist bits != tmax bits.
//
// The gather: k_gather_generate makes, for every (triangle, sample), a point on the triangle, a point on the lamp's rod (or
// on the rod swept along a segment), the ray between them and the sample's weight; k_occlude_free answers which samples see
// the lamp; k_gather_reduce sums the visible weights per triangle in sample order.  No atomics: the plane is a pure function
// of the arguments.  With the context's variance state on (uvrt_set_gather_variance) k_gather_reduce_var<MODE> takes
// k_gather_reduce's place: the same expected[t], and beside it the variance of that estimate from a second pass over the same
// samples.  This file is built without contraction, every operator below is one rounding.
#include "uvrt_query.h"

namespace uvrt {

// the answer of the ray a lane has finished
struct OccludedAnswer {
    const OccludeParams& op;
    __device__ __forceinline__ void operator()(const LaneF& L, float tmax, uint32_t slot) const
    {
        if (slot != NO_SLOT) op.occluded[slot] = __float_as_uint(L.po.y) != __float_as_uint(tmax) ? 1 : 0;
    }
};

template <int FL>
__global__ __launch_bounds__(256, FREE_GRID_PER_CU) void k_occlude_free(OccludeParams op)
{
    run_query_rays<FL, true>(op.e, op.oxz, op.tmax, OccludedAnswer{op});
}

bool launch_occlude_free(const OccludeParams& p, int grid_per_cu, hipStream_t s)
{
    return launch_query_free(p, k_occlude_free<0>, k_occlude_free<1>, grid_per_cu, s);
}

// ---- the direct gather ----

__global__ __launch_bounds__(256) void k_gather_tris(const LeafTri* __restrict__ ltris, float4* __restrict__ gtris, int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const LeafTri lt = ltris[i];
    const uint32_t id = __float_as_uint(lt.v0_id.w);
    if (id >= (uint32_t)T) return;
    gtris[(size_t)id * 3 + 0] = make_float4(lt.v0_id.x, lt.v0_id.y, lt.v0_id.z, 0.f);
    gtris[(size_t)id * 3 + 1] = make_float4(lt.e1.x, lt.e1.y, lt.e1.z, 0.f);
    gtris[(size_t)id * 3 + 2] = make_float4(lt.e2.x, lt.e2.y, lt.e2.z, 0.f);
}

void launch_gather_tris(const LeafTri* ltris, float4* gtris, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_gather_tris, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, ltris, gtris, T);
}

// MODE: the context's gather sampling (include/uvrt.h uvrt_set_gather_sampling).  0 is the independent rule; 1 puts sample s
// into stratum s of the rod and the sweep coordinate on a golden-ratio Weyl sequence rotated per triangle and seed.  The four
// draws are the same in both, so (a, b) are: only u_h and u_m differ.
template <int MODE>
__global__ __launch_bounds__(256) void k_gather_generate(GatherGenParams g)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.tri_count * g.samples) return;
    const uint32_t lt = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lt * g.samples);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const uint32_t j = t * (uint32_t)g.samples + s;
    uint32_t rng = wang_hash(j ^ g.seed_hash);
    float u_h = random_float(rng);
    float u_m = random_float(rng);
    if (MODE == 1) {
        u_h = ((float)s + u_h) / (float)g.samples;                          // jittered stratum s: two roundings
        const uint32_t h_t = wang_hash(t ^ wang_hash(g.seed ^ 0x9E3779B9u));    // once per thread: the triangle's rotation
        const uint32_t k = s * 0x9E3779B9u + h_t;                          // wraps
        u_m = (float)(k >> 8) * 5.9604644775390625e-8f;                     // 24 bits x 2^-24: exact
    }
    float a = random_float(rng);
    float b = random_float(rng);
    if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
    const float4 v0 = g.gtris[(size_t)t * 3 + 0], e1 = g.gtris[(size_t)t * 3 + 1], e2 = g.gtris[(size_t)t * 3 + 2];
    const float px = (v0.x + a * e1.x) + b * e2.x;
    const float py = (v0.y + a * e1.y) + b * e2.y;
    const float pz = (v0.z + a * e1.z) + b * e2.z;
    // k_generate_sweep's origin with r1 := u_h and u := u_m
    const float sx = g.tx - g.fx, sy = g.ty - g.fy, sz = g.tz - g.fz;
    const float ox = g.fx + u_m * sx;
    const float oy = (g.fy + u_h * g.light_length) + u_m * sy;
    const float oz = g.fz + u_m * sz;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
    double nx, ny, nz;
    const double nn = tri_normal(e1, e2, nx, ny, nz);
    const double Dx = (double)dx, Dy = (double)dy, Dz = (double)dz;
    const double R2 = Dx * Dx + Dy * Dy + Dz * Dz;
    const double R = sqrt(R2);
    double w = fabs(nx * Dx + ny * Dy + nz * Dz) / (nn * (R2 * R) * 12.566370614359172);
    float4 ray = make_float4(dx / r, dy / r, dz / r, oy);
    float tm = r * 0.9990234375f;
    if (!(r > 0.0f) || !(r <= 3.4028234663852886e38f)) {      // no direction: not traced (tmax 0 accepts no hit), weighs 0
        ray = make_float4(0.f, 1.f, 0.f, oy);
        tm = 0.0f;
        w = 0.0;
    }
    g.rays[i] = ray;
    g.oxz[i] = make_float2(ox, oz);
    g.tmax[i] = tm;
    g.w[i] = w;
}

void launch_gather_generate(const GatherGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.mode == 1) hipLaunchKernelGGL((k_gather_generate<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gather_generate<0>), grid, dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_gather_reduce(const float4* __restrict__ gtris, const double* __restrict__ w,
                                                       const uint8_t* __restrict__ occluded, double* __restrict__ expected,
                                                       int32_t first_tri, int32_t tri_count, int32_t samples, int32_t photons_equiv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tri_count) return;
    const size_t t = (size_t)first_tri + (size_t)i;
    double nx, ny, nz;
    const double nn = tri_normal(gtris[t * 3 + 1], gtris[t * 3 + 2], nx, ny, nz);
    double sum = 0.0;
    const size_t at = (size_t)i * (size_t)samples;
    for (int32_t s = 0; s < samples; ++s) sum = sum + (occluded[at + s] ? 0.0 : w[at + s]);
    expected[t] = nn == 0.0 ? 0.0 : ((double)photons_equiv * (0.5 * nn)) * (sum / (double)samples);
}

void launch_gather_reduce(const float4* gtris, const double* w, const uint8_t* occluded, double* expected, int32_t first_tri,
                          int32_t tri_count, int32_t samples, int32_t photons_equiv, hipStream_t s)
{
    if (tri_count <= 0) return;
    hipLaunchKernelGGL(k_gather_reduce, dim3((unsigned)((tri_count + 255) / 256)), dim3(256), 0, s, gtris, w, occluded, expected,
                       first_tri, tri_count, samples, photons_equiv);
}

// k_gather_reduce with the variance of the estimate beside it (include/uvrt.h uvrt_set_gather_variance): x_s = occluded ? 0 : w_s,
// `sum` and nn formed as above, so expected[t] carries the same bits; then a second pass over the samples in order.  MODE 0
// (independent samples): the sample variance of the mean, q = sum (x_s - m)^2 over S (S - 1).  MODE 1 (one sample per
// stratum of the rod): successive differences, q = sum (x_s - x_{s-1})^2 over 2 S (S - 1) -- the sample variance would charge
// the estimate for the rod's own trend, which stratification has already taken out.  samples >= 2.
template <int MODE>
__global__ __launch_bounds__(256) void k_gather_reduce_var(const float4* __restrict__ gtris, const double* __restrict__ w,
                                                           const uint8_t* __restrict__ occluded, double* __restrict__ expected,
                                                           double* __restrict__ variance, int32_t first_tri, int32_t tri_count,
                                                           int32_t samples, int32_t photons_equiv)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tri_count) return;
    const size_t t = (size_t)first_tri + (size_t)i;
    double nx, ny, nz;
    const double nn = tri_normal(gtris[t * 3 + 1], gtris[t * 3 + 2], nx, ny, nz);
    double sum = 0.0;
    const size_t at = (size_t)i * (size_t)samples;
    for (int32_t s = 0; s < samples; ++s) sum = sum + (occluded[at + s] ? 0.0 : w[at + s]);
    const double c = (double)photons_equiv * (0.5 * nn);
    const double m = sum / (double)samples;
    expected[t] = nn == 0.0 ? 0.0 : c * m;
    double q = 0.0;
    if (MODE == 0) {
        for (int32_t s = 0; s < samples; ++s) {
            const double d = (occluded[at + s] ? 0.0 : w[at + s]) - m;
            q = q + d * d;
        }
    } else {
        double prev = occluded[at] ? 0.0 : w[at];
        for (int32_t s = 1; s < samples; ++s) {
            const double x = occluded[at + s] ? 0.0 : w[at + s];
            const double d = x - prev;
            q = q + d * d;
            prev = x;
        }
    }
    const double SS = (double)samples * (double)(samples - 1);
    const double v = MODE == 0 ? q / SS : q / (2.0 * SS);
    variance[t] = nn == 0.0 ? 0.0 : (c * c) * v;
}

void launch_gather_reduce_var(const float4* gtris, const double* w, const uint8_t* occluded, double* expected, double* variance,
                              int32_t first_tri, int32_t tri_count, int32_t samples, int32_t photons_equiv, int32_t mode,
                              hipStream_t s)
{
    if (tri_count <= 0) return;
    const dim3 grid((unsigned)((tri_count + 255) / 256));
    if (mode == 1) hipLaunchKernelGGL((k_gather_reduce_var<1>), grid, dim3(256), 0, s, gtris, w, occluded, expected, variance,
                                      first_tri, tri_count, samples, photons_equiv);
    else hipLaunchKernelGGL((k_gather_reduce_var<0>), grid, dim3(256), 0, s, gtris, w, occluded, expected, variance, first_tri,
                            tri_count, samples, photons_equiv);
}

__global__ __launch_bounds__(256) void k_accumulate_expected(double* __restrict__ photon_map, double* __restrict__ max_map,
                                                             double* __restrict__ expected, float time_step, int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const double c = expected[i];
    photon_map[i] = photon_map[i] + c * (double)time_step;     // accumulate.cl:9
    const double m = max_map[i];
    max_map[i] = m < c ? c : m;
    expected[i] = 0.0;
}

void launch_accumulate_expected(double* photon_map, double* max_map, double* expected, float time_step, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_accumulate_expected, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, photon_map, max_map, expected,
                       time_step, T);
}

}  // namespace uvrt

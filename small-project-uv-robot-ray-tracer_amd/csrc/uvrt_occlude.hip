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
// samples.  The sample rule and the sums are uvrt_gather_sample.h's, which the batched gather
// (uvrt_gather_batch.hip) shares.  With the context's faces state on (uvrt_set_gather_faces) k_gather_generate_faces<MODE> takes
// k_gather_generate's place -- the same arrays and a byte per sample, the face it arrives on -- and k_gather_reduce_faces runs
// beside the reduce kernel of the state and writes the two face planes.
// This file is built without contraction, every operator is one rounding.
#include "uvrt_query.h"
#include "uvrt_gather_sample.h"

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

// One thread per (triangle, sample) of the chunk: the sample of uvrt_gather_sample.h (MODE: the context's gather sampling) into
// the chunk's arrays
template <int MODE>
__global__ __launch_bounds__(256) void k_gather_generate(GatherGenParams g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.tri_count * g.samples) return;
    const uint32_t lt = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lt * g.samples);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const GatherLamp l = {g.fx, g.fy, g.fz, g.tx, g.ty, g.tz, g.light_length, g.seed, g.seed_hash};
    const GatherSample o = gather_sample<MODE>(g.gtris, l, t, s, g.samples);
    g.rays[i] = o.ray;
    g.oxz[i] = o.oxz;
    g.tmax[i] = o.tmax;
    g.w[i] = o.w;
}

void launch_gather_generate(const GatherGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.mode == 1) hipLaunchKernelGGL((k_gather_generate<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_gather_generate<0>), grid, dim3(256), 0, s, p);
}

// k_gather_generate<MODE> that also keeps the face each sample arrives on (uvrt_gather_sample.h gather_face), a byte beside w:
// launched in its place while the context's faces state is on (include/uvrt.h uvrt_set_gather_faces)
template <int MODE>
__global__ __launch_bounds__(256) void k_gather_generate_faces(GatherGenParams g, uint8_t* __restrict__ face)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.tri_count * g.samples) return;
    const uint32_t lt = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lt * g.samples);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const GatherLamp l = {g.fx, g.fy, g.fz, g.tx, g.ty, g.tz, g.light_length, g.seed, g.seed_hash};
    const GatherSample o = gather_sample<MODE>(g.gtris, l, t, s, g.samples);
    g.rays[i] = o.ray;
    g.oxz[i] = o.oxz;
    g.tmax[i] = o.tmax;
    g.w[i] = o.w;
    face[i] = gather_face(o.c);
}

void launch_gather_generate_faces(const GatherGenParams& p, uint8_t* face, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.mode == 1) hipLaunchKernelGGL((k_gather_generate_faces<1>), grid, dim3(256), 0, s, p, face);
    else hipLaunchKernelGGL((k_gather_generate_faces<0>), grid, dim3(256), 0, s, p, face);
}

// The face planes: faces[f * T + t] = what k_gather_reduce gives from the samples that arrive on face f alone.  It runs beside
// the reduce kernel of the state (which writes expected[t], and variance[t], as ever), one thread per triangle, two sums in
// sample order.
__global__ __launch_bounds__(256) void k_gather_reduce_faces(const float4* __restrict__ gtris, const double* __restrict__ w,
                                                             const uint8_t* __restrict__ occluded, const uint8_t* __restrict__ face,
                                                             double* __restrict__ faces, int32_t first_tri, int32_t tri_count,
                                                             int32_t samples, int32_t photons_equiv, int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tri_count) return;
    const size_t t = (size_t)first_tri + (size_t)i;
    const double nn = gather_tri_nn(gtris, t);
    double sum0, sum1;
    gather_face_sums(w, occluded, face, (size_t)i * (size_t)samples, samples, sum0, sum1);
    faces[t] = gather_expected(nn, sum0, samples, photons_equiv);
    faces[(size_t)T + t] = gather_expected(nn, sum1, samples, photons_equiv);
}

void launch_gather_reduce_faces(const float4* gtris, const double* w, const uint8_t* occluded, const uint8_t* face, double* faces,
                                int32_t first_tri, int32_t tri_count, int32_t samples, int32_t photons_equiv, int32_t T, hipStream_t s)
{
    if (tri_count <= 0) return;
    hipLaunchKernelGGL(k_gather_reduce_faces, dim3((unsigned)((tri_count + 255) / 256)), dim3(256), 0, s, gtris, w, occluded, face,
                       faces, first_tri, tri_count, samples, photons_equiv, T);
}

__global__ __launch_bounds__(256) void k_gather_reduce(const float4* __restrict__ gtris, const double* __restrict__ w,
                                                       const uint8_t* __restrict__ occluded, double* __restrict__ expected,
                                                       int32_t first_tri, int32_t tri_count, int32_t samples, int32_t photons_equiv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tri_count) return;
    const size_t t = (size_t)first_tri + (size_t)i;
    const double nn = gather_tri_nn(gtris, t);
    const size_t at = (size_t)i * (size_t)samples;
    expected[t] = gather_expected(nn, gather_sum(w, occluded, at, samples), samples, photons_equiv);
}

void launch_gather_reduce(const float4* gtris, const double* w, const uint8_t* occluded, double* expected, int32_t first_tri,
                          int32_t tri_count, int32_t samples, int32_t photons_equiv, hipStream_t s)
{
    if (tri_count <= 0) return;
    hipLaunchKernelGGL(k_gather_reduce, dim3((unsigned)((tri_count + 255) / 256)), dim3(256), 0, s, gtris, w, occluded, expected,
                       first_tri, tri_count, samples, photons_equiv);
}

// k_gather_reduce with the variance of the estimate beside it (include/uvrt.h uvrt_set_gather_variance; uvrt_gather_sample.h
// gather_expected_var): expected[t] carries the same bits.  samples >= 2.
template <int MODE>
__global__ __launch_bounds__(256) void k_gather_reduce_var(const float4* __restrict__ gtris, const double* __restrict__ w,
                                                           const uint8_t* __restrict__ occluded, double* __restrict__ expected,
                                                           double* __restrict__ variance, int32_t first_tri, int32_t tri_count,
                                                           int32_t samples, int32_t photons_equiv)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= tri_count) return;
    const size_t t = (size_t)first_tri + (size_t)i;
    const double nn = gather_tri_nn(gtris, t);
    const size_t at = (size_t)i * (size_t)samples;
    gather_expected_var<MODE>(w, occluded, at, samples, nn, gather_sum(w, occluded, at, samples), photons_equiv, expected[t],
                              variance[t]);
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

// uvrt_mirror.hip -- the mirror gather's own kernels (include/uvrt.h "specular panels").  A chunk of one
// panel runs five steps on the context's stream: k_mirror_generate makes, for every (triangle, sample), leg A's ray from the
// lamp point to the mirror point, the image's weight, its face byte and the receiver point; k_closest_free
// (uvrt_indirect.hip, as it is) answers leg A; k_mirror_fold turns each hit record into leg B's ray, written over leg A's,
// or marks the sample lost with a zero weight; k_occlude_free (uvrt_occlude.hip, as it is) answers leg B; k_mirror_reduce
// sums per triangle in sample order with uvrt_gather_sample.h's sums.  No atomics, no loop beyond the S samples of a
// triangle: the plane is a pure function of the arguments.  The sample rule is uvrt_mirror_sample.h's.  This file is built
// without contraction, every operator is one rounding.
#include "uvrt_mirror_sample.h"

namespace uvrt {

template <int MODE>
__global__ __launch_bounds__(256) void k_mirror_generate(MirrorGenParams p)
{
    const GatherGenParams& g = p.g;
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.tri_count * g.samples) return;
    const uint32_t lt = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lt * g.samples);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const GatherLamp l = {g.fx, g.fy, g.fz, g.tx, g.ty, g.tz, g.light_length, g.seed, g.seed_hash};
    const MirrorSample o = mirror_sample<MODE>(g.gtris, l, p.m, t, s, g.samples);
    g.rays[i] = o.ray;
    g.oxz[i] = o.oxz;
    g.tmax[i] = o.tmax;
    g.w[i] = o.w;
    p.face[i] = gather_face(o.c);
    p.point[i] = make_float4(o.px, o.py, o.pz, 0.f);
}

void launch_mirror_generate(const MirrorGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.g.tri_count * p.g.samples;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.g.mode == 1) hipLaunchKernelGGL((k_mirror_generate<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_mirror_generate<0>), grid, dim3(256), 0, s, p);
}

// One thread per sample of the chunk, after the closest-hit launch has completed: leg B's ray over leg A's.  Nothing else
// reads or writes the arrays meanwhile.
__global__ __launch_bounds__(256) void k_mirror_fold(MirrorFoldParams f)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= f.n) return;
    float4 ray;
    float2 oxz;
    float tmax;
    const bool kept = mirror_fold(f.rays[i], f.oxz[i], f.hit[i], f.point[i], f.panel_of_tri, f.member, f.T, ray, oxz, tmax);
    f.rays[i] = ray;
    f.oxz[i] = oxz;
    f.tmax[i] = tmax;
    if (!kept) f.w[i] = 0.0;
}

void launch_mirror_fold(const MirrorFoldParams& p, hipStream_t s)
{
    if (p.n <= 0) return;
    hipLaunchKernelGGL(k_mirror_fold, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
}

// expected[t] = accumulate ? expected[t] + m[t] : m[t], m[t] what k_gather_reduce forms from the chunk's samples
__global__ __launch_bounds__(256) void k_mirror_reduce(MirrorReduceParams r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.tri_count) return;
    const size_t t = (size_t)r.first_tri + (size_t)i;
    const double nn = gather_tri_nn(r.gtris, t);
    const double m = gather_expected(nn, gather_sum(r.w, r.occluded, (size_t)i * (size_t)r.samples, r.samples), r.samples,
                                     r.photons_equiv);
    r.expected[t] = r.accumulate ? r.expected[t] + m : m;
}

// the same sum split by face into faces[f * T + t], under the same rule
__global__ __launch_bounds__(256) void k_mirror_reduce_faces(MirrorReduceParams r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.tri_count) return;
    const size_t t = (size_t)r.first_tri + (size_t)i;
    const double nn = gather_tri_nn(r.gtris, t);
    double sum0, sum1;
    gather_face_sums(r.w, r.occluded, r.face, (size_t)i * (size_t)r.samples, r.samples, sum0, sum1);
    const double m0 = gather_expected(nn, sum0, r.samples, r.photons_equiv);
    const double m1 = gather_expected(nn, sum1, r.samples, r.photons_equiv);
    double* f0 = r.faces + t;
    double* f1 = r.faces + (size_t)r.T + t;
    *f0 = r.accumulate ? *f0 + m0 : m0;
    *f1 = r.accumulate ? *f1 + m1 : m1;
}

void launch_mirror_reduce(const MirrorReduceParams& p, hipStream_t s)
{
    if (p.tri_count <= 0) return;
    const dim3 grid((unsigned)((p.tri_count + 255) / 256));
    hipLaunchKernelGGL(k_mirror_reduce, grid, dim3(256), 0, s, p);
    if (p.faces) hipLaunchKernelGGL(k_mirror_reduce_faces, grid, dim3(256), 0, s, p);
}

}  // namespace uvrt

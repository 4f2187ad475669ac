// uvrt_gather_sample.h -- the direct gather's sample and its per-triangle sums (include/uvrt.h "shadow rays and the direct
// gather"), as the launch-by-launch kernels (uvrt_occlude.hip) and the batched ones (uvrt_gather_batch.hip) both form them:
// one copy of every expression, so the two cannot drift apart.  Both files are built without contraction, every operator
// below is one rounding.
#pragma once
#include "uvrt_device.h"

namespace uvrt {

// the lamp of one gather launch as the sample rule reads it
struct GatherLamp {
    float fx, fy, fz, tx, ty, tz;
    float light_length;
    uint32_t seed;           // the raw seed: the stratified rule hashes it again for the triangle's rotation
    uint32_t seed_hash;      // WangHash(seed)
};

// what a sample leaves in the chunk's arrays
struct GatherSample {
    float4 ray;              // dir.xyz, orig.y
    float2 oxz;              // orig.x, orig.z
    float tmax;
    double w;                // the sample's weight (0 for a sample that is not traced)
    double c;                // n.D, the value w takes fabs of: its sign is the face the sample arrives on (gather_face)
    float dx, dy, dz, r;     // D = p - source point in f32 and its f32 length, before the division
};

// The two points of a sample: p on the triangle, o on the lamp's rod (or on the rod swept along the segment), and the
// triangle's edges for the normal.  What the direct gather and the mirror gather (uvrt_mirror_sample.h) both start from.
struct GatherPoints {
    float px, py, pz;
    float ox, oy, oz;
    float4 e1, e2;
};

// The points of sample s of `samples` of triangle t.  MODE: the gather sampling (include/uvrt.h uvrt_set_gather_sampling).  0 is
// the independent rule; 1 puts sample s into stratum s of the rod and the sweep coordinate on a golden-ratio Weyl sequence
// rotated per triangle and seed.  The four draws are the same in both, so (a, b) are: only u_h and u_m differ.
template <int MODE>
__device__ __forceinline__ GatherPoints gather_points(const float4* __restrict__ gtris, const GatherLamp& l, uint32_t t, uint32_t s,
                                                      int32_t samples)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const uint32_t j = t * (uint32_t)samples + s;
    uint32_t rng = wang_hash(j ^ l.seed_hash);
    float u_h = random_float(rng);
    float u_m = random_float(rng);
    if (MODE == 1) {
        u_h = ((float)s + u_h) / (float)samples;                            // jittered stratum s: two roundings
        const uint32_t h_t = wang_hash(t ^ wang_hash(l.seed ^ 0x9E3779B9u));    // once per thread: the triangle's rotation
        const uint32_t k = s * 0x9E3779B9u + h_t;                          // wraps
        u_m = (float)(k >> 8) * 5.9604644775390625e-8f;                     // 24 bits x 2^-24: exact
    }
    float a = random_float(rng);
    float b = random_float(rng);
    if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
    const float4 v0 = gtris[(size_t)t * 3 + 0], e1 = gtris[(size_t)t * 3 + 1], e2 = gtris[(size_t)t * 3 + 2];
    GatherPoints g;
    g.px = (v0.x + a * e1.x) + b * e2.x;
    g.py = (v0.y + a * e1.y) + b * e2.y;
    g.pz = (v0.z + a * e1.z) + b * e2.z;
    // k_generate_sweep's origin with r1 := u_h and u := u_m
    const float sx = l.tx - l.fx, sy = l.ty - l.fy, sz = l.tz - l.fz;
    g.ox = l.fx + u_m * sx;
    g.oy = (l.fy + u_h * l.light_length) + u_m * sy;
    g.oz = l.fz + u_m * sz;
    g.e1 = e1;
    g.e2 = e2;
    return g;
}

// The ray from the source point (ox, oy, oz) to the sample's point p, its weight and the n.D the weight takes fabs of.  The
// direct gather's source point is the sample's own o; the mirror gather's is o's image behind a panel.
__device__ __forceinline__ GatherSample gather_weigh(const GatherPoints& g, float ox, float oy, float oz)
{
    const float dx = g.px - ox, dy = g.py - oy, dz = g.pz - oz;
    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
    double nx, ny, nz;
    const double nn = tri_normal(g.e1, g.e2, nx, ny, nz);
    const double Dx = (double)dx, Dy = (double)dy, Dz = (double)dz;
    const double R2 = Dx * Dx + Dy * Dy + Dz * Dz;
    const double R = sqrt(R2);
    GatherSample o;
    o.dx = dx; o.dy = dy; o.dz = dz; o.r = r;
    o.c = nx * Dx + ny * Dy + nz * Dz;
    o.w = fabs(o.c) / (nn * (R2 * R) * 12.566370614359172);
    o.ray = make_float4(dx / r, dy / r, dz / r, oy);
    o.tmax = r * 0.9990234375f;
    if (!(r > 0.0f) || !(r <= 3.4028234663852886e38f)) {      // no direction: not traced (tmax 0 accepts no hit), weighs 0
        o.ray = make_float4(0.f, 1.f, 0.f, oy);
        o.tmax = 0.0f;
        o.w = 0.0;
    }
    o.oxz = make_float2(ox, oz);
    return o;
}

// Sample s of `samples` of triangle t of the direct gather: the ray from its lamp point to its point on the triangle
template <int MODE>
__device__ __forceinline__ GatherSample gather_sample(const float4* __restrict__ gtris, const GatherLamp& l, uint32_t t, uint32_t s,
                                                      int32_t samples)
{
    const GatherPoints g = gather_points<MODE>(gtris, l, t, s, samples);
    return gather_weigh(g, g.ox, g.oy, g.oz);
}

// |cross(e1, e2)| of triangle t
__device__ __forceinline__ double gather_tri_nn(const float4* __restrict__ gtris, size_t t)
{
    double nx, ny, nz;
    return tri_normal(gtris[t * 3 + 1], gtris[t * 3 + 2], nx, ny, nz);
}

// the visible weights of the `samples` samples behind `at`, in sample order
__device__ __forceinline__ double gather_sum(const double* __restrict__ w, const uint8_t* __restrict__ occluded, size_t at,
                                             int32_t samples)
{
    double sum = 0.0;
    for (int32_t s = 0; s < samples; ++s) sum = sum + (occluded[at + s] ? 0.0 : w[at + s]);
    return sum;
}

// expected[t] from the sum
__device__ __forceinline__ double gather_expected(double nn, double sum, int32_t samples, int32_t photons_equiv)
{
    return nn == 0.0 ? 0.0 : ((double)photons_equiv * (0.5 * nn)) * (sum / (double)samples);
}

// The face a sample arrives on (include/uvrt.h "face-resolved gather and bounces"): face 0 is the side n = cross(e1, e2) points
// to, and light travelling along D reaches it iff n.D < 0.  c is GatherSample::c (a NaN, from a sample that weighs 0, counts
// as face 1).
__device__ __forceinline__ uint8_t gather_face(double c)
{
    return c < 0.0 ? (uint8_t)0 : (uint8_t)1;
}

// gather_sum split by the face of each sample: sum0 + sum1 visit the samples gather_sum visits, each in sample order from
// +0.0 (a sample of the other face is skipped: every term is >= +0, so adding +0.0 for it would leave the same bits)
__device__ __forceinline__ void gather_face_sums(const double* __restrict__ w, const uint8_t* __restrict__ occluded,
                                                 const uint8_t* __restrict__ face, size_t at, int32_t samples, double& sum0,
                                                 double& sum1)
{
    sum0 = 0.0;
    sum1 = 0.0;
    for (int32_t s = 0; s < samples; ++s) {
        const double x = occluded[at + s] ? 0.0 : w[at + s];
        if (face[at + s]) sum1 = sum1 + x;
        else sum0 = sum0 + x;
    }
}

// expected[t] (the bits of gather_expected) and the variance of that estimate from a second pass over the samples in order
// (include/uvrt.h uvrt_set_gather_variance): x_s = occluded ? 0 : w_s.  MODE 0 (independent samples): the sample variance of the
// mean, q = sum (x_s - m)^2 over S (S - 1).  MODE 1 (one sample per stratum of the rod): successive differences,
// q = sum (x_s - x_{s-1})^2 over 2 S (S - 1) -- the sample variance would charge the estimate for the rod's own trend, which
// stratification has already taken out.  samples >= 2.
template <int MODE>
__device__ __forceinline__ void gather_expected_var(const double* __restrict__ w, const uint8_t* __restrict__ occluded, size_t at,
                                                    int32_t samples, double nn, double sum, int32_t photons_equiv,
                                                    double& expected, double& variance)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const double c = (double)photons_equiv * (0.5 * nn);
    const double m = sum / (double)samples;
    expected = nn == 0.0 ? 0.0 : c * m;
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
    variance = nn == 0.0 ? 0.0 : (c * c) * v;
}

}  // namespace uvrt

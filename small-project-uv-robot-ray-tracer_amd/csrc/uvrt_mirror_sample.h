// uvrt_mirror_sample.h -- the sample of the mirror gather (include/uvrt.h "specular panels"): the
// direct gather's sample (uvrt_gather_sample.h gather_points / gather_weigh) seen in a planar panel.  The receiver sees the
// lamp point o mirrored in the panel's plane, o', at the unfolded distance: the weight and the face are gather_weigh's with o'
// in place of o.  Two legs are traced for it: A from o to the mirror point P (a closest hit: it must end on a member triangle
// of the panel), B from the point that hit found to the receiver (an occlusion query).  Built without contraction, every
// operator below is one rounding.
#pragma once
#include "uvrt_gather_sample.h"

namespace uvrt {

// what a sample leaves in the chunk's arrays for leg A
struct MirrorSample {
    float4 ray;              // leg A: dir.xyz, orig.y
    float2 oxz;
    float tmax;              // 1e30f, or 0 for a sample that is not traced
    double w;                // rho * the image's weight (0 for a sample that is not traced)
    double c;                // n.D' (gather_face)
    float px, py, pz;        // the receiver point
};

__device__ __forceinline__ bool mirror_finite(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// signed distance of the f32 point (x, y, z) from the panel's plane, along its normal
__device__ __forceinline__ double mirror_side(const MirrorPanel& m, float x, float y, float z)
{
    return (((double)x - m.qx) * m.mx + ((double)y - m.qy) * m.my) + ((double)z - m.qz) * m.mz;
}

template <int MODE>
__device__ __forceinline__ MirrorSample mirror_sample(const float4* __restrict__ gtris, const GatherLamp& l, const MirrorPanel& m,
                                                      uint32_t t, uint32_t s, int32_t samples)
{
    const GatherPoints g = gather_points<MODE>(gtris, l, t, s, samples);
    MirrorSample o;
    o.px = g.px; o.py = g.py; o.pz = g.pz;
    o.ray = make_float4(0.f, 1.f, 0.f, g.oy);       // not traced: tmax 0 accepts no hit
    o.oxz = make_float2(g.ox, g.oz);
    o.tmax = 0.0f;
    o.w = 0.0;
    o.c = 0.0;
    const double d_o = mirror_side(m, g.ox, g.oy, g.oz);
    const double d_p = mirror_side(m, g.px, g.py, g.pz);
    if (!(d_o > 0.0) || !(d_p > 0.0)) return o;     // the lamp point or the receiver is not in front of the panel
    const double two = 2.0 * d_o;
    const float ix = (float)((double)g.ox - two * m.mx);
    const float iy = (float)((double)g.oy - two * m.my);
    const float iz = (float)((double)g.oz - two * m.mz);
    const GatherSample q = gather_weigh(g, ix, iy, iz);
    o.c = q.c;
    if (!(q.r > 0.0f) || !(q.r <= 3.4028234663852886e38f)) return o;       // gather_weigh's degenerate distance: weighs 0
    // the mirror point: where the unfolded segment o' -> p crosses the plane
    const double tau = d_o / (d_o + d_p);
    const float Px = (float)((double)ix + tau * (double)q.dx);
    const float Py = (float)((double)iy + tau * (double)q.dy);
    const float Pz = (float)((double)iz + tau * (double)q.dz);
    const float ax = Px - g.ox, ay = Py - g.oy, az = Pz - g.oz;
    const float ra = sqrtf((ax * ax + ay * ay) + az * az);
    if (!(ra > 0.0f) || !mirror_finite(ra)) return o;
    o.ray = make_float4(ax / ra, ay / ra, az / ra, g.oy);
    o.tmax = 1e30f;
    o.w = m.rho * q.w;
    return o;
}

// Leg B of a sample from leg A's ray (dir, origin), its closest hit (dist bits, triangle) and the receiver point p.  Returns
// false for a lost sample: leg A did not end on a member triangle of the panel, or leg B has no direction.
__device__ __forceinline__ bool mirror_fold(const float4 rayA, const float2 oxzA, const uint2 hit, const float4 p,
                                            const uint8_t* __restrict__ panel_of_tri, int32_t member, int32_t T, float4& rayB,
                                            float2& oxzB, float& tmaxB)
{
    rayB = make_float4(0.f, 1.f, 0.f, rayA.w);
    oxzB = oxzA;
    tmaxB = 0.0f;
    if (!(hit.y < (uint32_t)T) || (int32_t)panel_of_tri[hit.y] != member) return false;
    const float dist = __uint_as_float(hit.x);
    const float hx = oxzA.x + dist * rayA.x;
    const float hy = rayA.w + dist * rayA.y;
    const float hz = oxzA.y + dist * rayA.z;
    const float bx = p.x - hx, by = p.y - hy, bz = p.z - hz;
    const float rb = sqrtf((bx * bx + by * by) + bz * bz);
    if (!(rb > 0.0f) || !mirror_finite(rb)) return false;
    rayB = make_float4(bx / rb, by / rb, bz / rb, hy + by * 0.0009765625f);
    oxzB = make_float2(hx + bx * 0.0009765625f, hz + bz * 0.0009765625f);
    tmaxB = rb * 0.998046875f;
    return true;
}

}  // namespace uvrt

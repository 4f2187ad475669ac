// uvrt_sensor_sample.h -- the sample rules of a receiver that is no triangle (include/uvrt.h "sensors"):
// the direct sample of a sensor (a lamp point, the ray to the sensor's position and its weight) and the reflected sample (a
// direction about a planar sensor's normal, or over the whole sphere of a spherical one).  A sensor draws two numbers for
// its lamp point where a triangle draws four, so the points are formed here and not by uvrt_gather_sample.h's
// gather_points; the lamp-point expressions are the same, operator for operator.  uvrt_sensors.hip is built without
// contraction, every operator below is one rounding.
#pragma once
#include "uvrt_gather_sample.h"

namespace uvrt {

// a sensor as the kernels read it
struct SensorRec {
    float px, py, pz;
    float nx, ny, nz;
    int32_t kind;            // UVRT_SENSOR_PLANAR (0) / UVRT_SENSOR_SPHERICAL (1)
};

__device__ __forceinline__ SensorRec sensor_load(const float4* __restrict__ sensors, size_t k)
{
    const float4 a = sensors[k * 2 + 0], b = sensors[k * 2 + 1];
    SensorRec r;
    r.px = a.x; r.py = a.y; r.pz = a.z;
    r.nx = a.w; r.ny = b.x; r.nz = b.y;
    r.kind = (int32_t)__float_as_uint(b.z);
    return r;
}

// what a direct sample leaves in the chunk's arrays
struct SensorSample {
    float4 ray;              // dir.xyz, orig.y
    float2 oxz;              // orig.x, orig.z
    float tmax;
    double w;
};

// Sample s of `samples` of sensor k: the lamp point o (k_generate_sweep's origin with r1 := u_h, u := u_m, as gather_points
// forms it), the ray from o to the sensor and the weight of what arrives there.  A planar sensor is one-sided: light
// travelling along D arrives on the side its normal points to iff n.D < 0.
template <int MODE>
__device__ __forceinline__ SensorSample sensor_sample(const SensorRec& r, const GatherLamp& l, uint32_t k, uint32_t s, int32_t samples)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const uint32_t j = k * (uint32_t)samples + s;
    uint32_t rng = wang_hash(j ^ l.seed_hash);
    float u_h = random_float(rng);
    float u_m = random_float(rng);
    if (MODE == 1) {
        u_h = ((float)s + u_h) / (float)samples;                            // jittered stratum s: two roundings
        const uint32_t h_k = wang_hash(k ^ wang_hash(l.seed ^ 0x9E3779B9u));    // the sensor's rotation
        const uint32_t m = s * 0x9E3779B9u + h_k;                          // wraps
        u_m = (float)(m >> 8) * 5.9604644775390625e-8f;                     // 24 bits x 2^-24: exact
    }
    const float sx = l.tx - l.fx, sy = l.ty - l.fy, sz = l.tz - l.fz;
    const float ox = l.fx + u_m * sx;
    const float oy = (l.fy + u_h * l.light_length) + u_m * sy;
    const float oz = l.fz + u_m * sz;
    const float dx = r.px - ox, dy = r.py - oy, dz = r.pz - oz;
    const float len = sqrtf((dx * dx + dy * dy) + dz * dz);
    const double Dx = (double)dx, Dy = (double)dy, Dz = (double)dz;
    const double R2 = (Dx * Dx + Dy * Dy) + Dz * Dz;
    const double R = sqrt(R2);
    double w;
    if (r.kind == 0) {
        const double nx = (double)r.nx, ny = (double)r.ny, nz = (double)r.nz;
        const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
        const double c = (nx * Dx + ny * Dy) + nz * Dz;
        w = c < 0.0 ? (-c) / (nn * (R2 * R) * 12.566370614359172) : 0.0;
    } else {
        w = 1.0 / (R2 * 12.566370614359172);
    }
    SensorSample o;
    o.ray = make_float4(dx / len, dy / len, dz / len, oy);
    o.tmax = len * 0.9990234375f;
    o.w = w;
    // no direction, or nothing to arrive: not traced (tmax 0 accepts no hit), weighs 0
    if (!(len > 0.0f) || !(len <= 3.4028234663852886e38f) || !(w > 0.0)) {
        o.ray = make_float4(0.f, 1.f, 0.f, oy);
        o.tmax = 0.0f;
        o.w = 0.0;
    }
    o.oxz = make_float2(ox, oz);
    return o;
}

// density[k] and variance[k] from the sum of the visible weights: gather_expected_var's two forms with c = photons_equiv and
// no area (a sensor's unit is expected photons per square metre).  samples == 1: the variance is 0.
template <int MODE>
__device__ __forceinline__ void sensor_density_var(const double* __restrict__ w, const uint8_t* __restrict__ occluded, size_t at,
                                                   int32_t samples, double sum, int32_t photons_equiv, double& density,
                                                   double& variance)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const double c = (double)photons_equiv;
    const double m = sum / (double)samples;
    density = c * m;
    variance = 0.0;
    if (samples < 2) return;
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
    variance = (c * c) * v;
}

__device__ __forceinline__ bool sensor_finite_f32(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

// Reflected sample s of `samples` of sensor k: a point (x, y) of the unit disc by uvrt_gather_indirect's bounded rejection,
// lifted to a cosine-distributed direction about a planar sensor's normal (all samples leave on the normal's side) or, by
// Marsaglia's map, to a uniform direction on a spherical sensor's sphere.  The ray starts at the sensor.
__device__ __forceinline__ void sensor_indirect_sample(const SensorRec& r, uint32_t seed_hash, uint32_t k, uint32_t s, int32_t samples,
                                                       float4& ray, float2& oxz, float& tmax)
{
    const uint32_t j = k * (uint32_t)samples + s;
    uint32_t rng = wang_hash(j ^ seed_hash);
    double x = 0.0, y = 0.0;
    for (int round = 0; round < 8; ++round) {
        const float xf = random_float(rng);
        const float yf = random_float(rng);
        const double xd = (double)(xf * 2.0f - 1.0f), yd = (double)(yf * 2.0f - 1.0f);
        if (xd * xd + yd * yd <= 1.0) { x = xd; y = yd; break; }
    }
    const double q = x * x + y * y;
    double Dx, Dy, Dz;
    bool ok = true;
    if (r.kind == 0) {
        const double z = sqrt(1.0 - q);
        const double nx = (double)r.nx, ny = (double)r.ny, nz = (double)r.nz;
        const double nn = sqrt((nx * nx + ny * ny) + nz * nz);
        const double ax = fabs(nx), ay = fabs(ny), az = fabs(nz);
        // cross(a, n) for a the unit axis of the smallest |n| component (x before y before z)
        double cx, cy, cz;
        if (ax <= ay && ax <= az) { cx = 0.0; cy = -nz; cz = ny; }
        else if (ay <= az) { cx = nz; cy = 0.0; cz = -nx; }
        else { cx = -ny; cy = nx; cz = 0.0; }
        const double cl = sqrt((cx * cx + cy * cy) + cz * cz);
        const double Tx = cx / cl, Ty = cy / cl, Tz = cz / cl;
        const double Bx = (ny * Tz - nz * Ty) / nn, By = (nz * Tx - nx * Tz) / nn, Bz = (nx * Ty - ny * Tx) / nn;
        const double zz = z / nn;
        Dx = ((x * Tx) + (y * Bx)) + (zz * nx);
        Dy = ((x * Ty) + (y * By)) + (zz * ny);
        Dz = ((x * Tz) + (y * Bz)) + (zz * nz);
        ok = nn != 0.0;
    } else {
        const double g = sqrt(1.0 - q);
        Dx = (2.0 * x) * g;
        Dy = (2.0 * y) * g;
        Dz = 1.0 - 2.0 * q;
    }
    const float dx = (float)Dx, dy = (float)Dy, dz = (float)Dz;
    ray = make_float4(dx, dy, dz, r.py);
    tmax = 1e30f;
    if (!ok || !sensor_finite_f32(dx) || !sensor_finite_f32(dy) || !sensor_finite_f32(dz) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        ray = make_float4(0.f, 1.f, 0.f, r.py);     // not traced: tmax 0 accepts no hit
        tmax = 0.0f;
    }
    oxz = make_float2(r.px, r.pz);
}

}  // namespace uvrt

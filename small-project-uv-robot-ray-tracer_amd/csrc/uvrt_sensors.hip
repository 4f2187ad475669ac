// uvrt_sensors.hip -- the kernels of the virtual dosimeters (include/uvrt.h "sensors").  A chunk of the
// direct call runs three steps on the context's stream: k_sensor_generate makes, for every (sensor, sample), the ray from
// its lamp point to the sensor and its weight; k_occlude_free (uvrt_occlude.hip, as it is) answers; k_sensor_reduce sums per
// sensor in sample order.  The reflected call: k_sensor_indirect_generate makes a ray from the sensor, k_closest_free
// (uvrt_indirect.hip, as it is) finds what it sees, k_sensor_indirect_reduce looks up the emitter's plane at the hit
// triangles.  No atomics, no LDS, no loop beyond the samples of a sensor: the planes are pure functions of the arguments.
// The sample rules are uvrt_sensor_sample.h's.  This file is built without contraction, every operator is one rounding.
#include "uvrt_sensor_sample.h"

namespace uvrt {

template <int MODE>
__global__ __launch_bounds__(256) void k_sensor_generate(SensorGenParams g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.count * g.samples) return;
    const uint32_t lk = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lk * g.samples);
    const uint32_t k = (uint32_t)g.first + lk;
    const GatherLamp l = {g.fx, g.fy, g.fz, g.tx, g.ty, g.tz, g.light_length, g.seed, g.seed_hash};
    const SensorSample o = sensor_sample<MODE>(sensor_load(g.sensors, k), l, k, s, g.samples);
    g.rays[i] = o.ray;
    g.oxz[i] = o.oxz;
    g.tmax[i] = o.tmax;
    g.w[i] = o.w;
}

void launch_sensor_generate(const SensorGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.count * p.samples;
    if (n <= 0) return;
    const dim3 grid((unsigned)((n + 255) / 256));
    if (p.mode == 1) hipLaunchKernelGGL((k_sensor_generate<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_sensor_generate<0>), grid, dim3(256), 0, s, p);
}

template <int MODE>
__global__ __launch_bounds__(256) void k_sensor_reduce(SensorReduceParams r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.count) return;
    const size_t k = (size_t)r.first + (size_t)i;
    const size_t at = (size_t)i * (size_t)r.samples;
    double density, variance;
    sensor_density_var<MODE>(r.w, r.occluded, at, r.samples, gather_sum(r.w, r.occluded, at, r.samples), r.photons_equiv, density,
                             variance);
    r.density[k] = density;
    r.variance[k] = variance;
}

void launch_sensor_reduce(const SensorReduceParams& p, hipStream_t s)
{
    if (p.count <= 0) return;
    const dim3 grid((unsigned)((p.count + 255) / 256));
    if (p.mode == 1) hipLaunchKernelGGL((k_sensor_reduce<1>), grid, dim3(256), 0, s, p);
    else hipLaunchKernelGGL((k_sensor_reduce<0>), grid, dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_sensor_indirect_generate(SensorGenParams g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.count * g.samples) return;
    const uint32_t lk = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lk * g.samples);
    const uint32_t k = (uint32_t)g.first + lk;
    float4 ray;
    float2 oxz;
    float tmax;
    sensor_indirect_sample(sensor_load(g.sensors, k), g.seed_hash, k, s, g.samples, ray, oxz, tmax);
    g.rays[i] = ray;
    g.oxz[i] = oxz;
    g.tmax[i] = tmax;
}

void launch_sensor_indirect_generate(const SensorGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.count * p.samples;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_sensor_indirect_generate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
}

// One thread per sensor: the radiosity each of its rays sees, in sample order.  Emitter 0 reads the source plane under one
// reflectance; emitter 1 reads the face plane of the face the ray arrives on (n_h . dir < 0: face 0, as the sided links
// decide it) under one reflectance or the map's.
__global__ __launch_bounds__(256) void k_sensor_indirect_reduce(SensorIndirectReduceParams r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.count) return;
    const size_t k = (size_t)r.first + (size_t)i;
    const size_t at = (size_t)i * (size_t)r.samples;
    const int32_t kind = sensor_load(r.sensors, k).kind;
    double sum = 0.0;
    for (int32_t s = 0; s < r.samples; ++s) {
        const uint32_t h = r.hit[at + s].y;
        double ys = 0.0;
        if (h < (uint32_t)r.T) {                            // (NO_TRI, a miss, is no triangle's id)
            double nx, ny, nz;
            const double nh = tri_normal(r.gtris[(size_t)h * 3 + 1], r.gtris[(size_t)h * 3 + 2], nx, ny, nz);
            if (nh > 0.0) {
                if (r.emitter == 0) {
                    ys = (double)r.reflectance * (r.source[h] / (0.5 * nh));
                } else {
                    const float4 d = r.rays[at + s];
                    const double c = (nx * (double)d.x + ny * (double)d.y) + nz * (double)d.z;
                    const size_t a = c < 0.0 ? (size_t)0 : (size_t)1;
                    const size_t e = a * (size_t)r.T + (size_t)h;
                    const double rho = r.use_map ? (double)r.rho[e] : (double)r.reflectance;
                    ys = rho * (r.faces[e] / (0.5 * nh));
                }
            }
        }
        sum = sum + ys;
    }
    const double ind = kind == 0 ? sum / (double)r.samples : (4.0 * sum) / (double)r.samples;
    r.density[k] = r.density[k] + ind;
}

void launch_sensor_indirect_reduce(const SensorIndirectReduceParams& p, hipStream_t s)
{
    if (p.count <= 0) return;
    hipLaunchKernelGGL(k_sensor_indirect_reduce, dim3((unsigned)((p.count + 255) / 256)), dim3(256), 0, s, p);
}

// accumulate.cl:4-14 per sensor, with the variance beside it: planes f64[5][K] = density, variance, dose_map, max_map, var_map
__global__ __launch_bounds__(256) void k_sensor_accumulate(double* __restrict__ planes, int32_t K, float time_step)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= K) return;
    const size_t n = (size_t)K;
    const double c = planes[i], v = planes[n + i];
    const double dt = (double)time_step;
    planes[2 * n + i] = planes[2 * n + i] + c * dt;
    const double m = planes[3 * n + i];
    planes[3 * n + i] = m < c ? c : m;
    planes[4 * n + i] = planes[4 * n + i] + v * (dt * dt);
    planes[i] = 0.0;
    planes[n + i] = 0.0;
}

void launch_sensor_accumulate(double* planes, int32_t K, float time_step, hipStream_t s)
{
    if (K <= 0) return;
    hipLaunchKernelGGL(k_sensor_accumulate, dim3((unsigned)((K + 255) / 256)), dim3(256), 0, s, planes, K, time_step);
}

// k_compute_dosage's arithmetic with area = 1.0f
__global__ __launch_bounds__(256) void k_sensor_dosage(const double* __restrict__ map, float* __restrict__ out, int32_t photons_per_light,
                                                       float scaled_power, int32_t first, int32_t count)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const double num = (double)scaled_power * map[(size_t)first + (size_t)i];
    const float den = 1.0f * (float)photons_per_light;
    out[i] = (float)(num / (double)den);
}

void launch_sensor_dosage(const double* map, float* out, int32_t photons_per_light, float scaled_power, int32_t first, int32_t count,
                          hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_sensor_dosage, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, map, out, photons_per_light,
                       scaled_power, first, count);
}

}  // namespace uvrt

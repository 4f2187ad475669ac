// uvrt_capi_sensors.hip -- virtual dosimeters (include/uvrt.h "sensors"): uvrt_set_sensors, uvrt_sensor_info,
// uvrt_read_sensors, uvrt_drop_sensors, uvrt_gather_sensors, uvrt_gather_sensors_indirect, uvrt_accumulate_sensors,
// uvrt_reset_sensors, uvrt_read_sensor_plane, uvrt_write_sensor_plane, uvrt_sensor_dosage (uvrt_sensors.hip's kernels around the
// shadow-ray and closest-hit launches of uvrt_capi_gather.hip and uvrt_capi_indirect.hip)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace {

constexpr int kSensorPlanes = 5;

double* sensor_plane(uvrt_ctx* c, int which)
{
    return c->sensor_planes.as<double>() + (size_t)which * (size_t)c->sensor_count;
}

// what the two tracing calls check alike; S is the call's sample count, already checked against its own limits
int check_sensor_trace(uvrt_ctx* c, int32_t first, int32_t count, int32_t S, const char* who)
{
    if (c->sensor_count <= 0) return fail(UVRT_ERR_INVALID, "%s: no sensors (uvrt_set_sensors)", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "%s: sensor rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", who, c->flavour);
    if (first < 0 || count < 0 || (int64_t)first + count > c->sensor_count)
        return fail(UVRT_ERR_INVALID, "%s: sensors [%d, +%d) outside [0, %d]", who, first, count, c->sensor_count);
    if ((int64_t)S > c->capacity)
        return fail(UVRT_ERR_INVALID, "%s: samples = %d exceed the ray capacity %lld (uvrt_resize_rays)", who, S, (long long)c->capacity);
    if ((int64_t)c->sensor_count * S >= ((int64_t)1 << 31))
        return fail(UVRT_ERR_INVALID, "%s: %d sensors x %d samples do not fit 2^31 sample numbers", who, c->sensor_count, S);
    return UVRT_OK;
}

int sensor_plane_range(uvrt_ctx* c, const char* who, int32_t which, void* host, int32_t first, int32_t count, hipMemcpyKind kind)
{
    if (!c || !host) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (c->sensor_count <= 0) return fail(UVRT_ERR_INVALID, "%s: no sensors (uvrt_set_sensors)", who);
    if (which < 0 || which >= kSensorPlanes) return fail(UVRT_ERR_INVALID, "%s: plane must be in [0, 4], not %d", who, which);
    if (!range_ok(host, first, count, c->sensor_count))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->sensor_count);
    return range_copy(c, sensor_plane(c, which), 8, host, first, count, kind);
}

}  // namespace

extern "C" {

int uvrt_set_sensors(uvrt_ctx* c, const uvrt_sensor* sensors, int32_t count)
{
    const char* who = "uvrt_set_sensors";
    if (!c || !sensors) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (count < 1 || count > UVRT_SENSOR_MAX)
        return fail(UVRT_ERR_INVALID, "%s: count = %d must be in [1, %d]", who, count, UVRT_SENSOR_MAX);
    for (int32_t k = 0; k < count; ++k) {
        const uvrt_sensor& s = sensors[k];
        if (s.kind != UVRT_SENSOR_PLANAR && s.kind != UVRT_SENSOR_SPHERICAL)
            return fail(UVRT_ERR_INVALID, "%s: sensor %d: kind must be 0 (planar) or 1 (spherical), not %d", who, k, s.kind);
        if (s.reserved != 0) return fail(UVRT_ERR_INVALID, "%s: sensor %d: reserved must be 0", who, k);
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(s.pos[a]) || !std::isfinite(s.normal[a]))
                return fail(UVRT_ERR_INVALID, "%s: sensor %d has a non-finite position or normal", who, k);
        if (s.kind == UVRT_SENSOR_PLANAR && s.normal[0] == 0.0f && s.normal[1] == 0.0f && s.normal[2] == 0.0f)
            return fail(UVRT_ERR_INVALID, "%s: sensor %d is planar and has a zero normal", who, k);
    }
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));       // nothing outstanding reads the buffers that are replaced below
    DevBuf recs, planes, out;
    if (int rc = recs.ensure((size_t)count * sizeof(uvrt_sensor), false, c->stream)) return rc;
    if (int rc = planes.ensure((size_t)count * 8 * kSensorPlanes, true, c->stream)) return rc;
    if (int rc = out.ensure((size_t)count * 4, false, c->stream)) return rc;
    if (int rc = copy_sync(c, recs.p, sensors, (size_t)count * sizeof(uvrt_sensor), hipMemcpyHostToDevice)) return rc;
    c->sensors.assign(sensors, sensors + count);
    c->sensors_dev = std::move(recs);
    c->sensor_planes = std::move(planes);
    c->sensor_out = std::move(out);
    c->sensor_count = count;
    return UVRT_OK;
}

int uvrt_sensor_info(uvrt_ctx* c, int32_t out4[4])
{
    if (!c || !out4) return fail(UVRT_ERR_INVALID, "uvrt_sensor_info: null argument");
    out4[0] = c->sensor_count;
    out4[1] = 0;
    out4[2] = 0;
    out4[3] = 0;
    return UVRT_OK;
}

int uvrt_read_sensors(uvrt_ctx* c, uvrt_sensor* sensors_out)
{
    if (!c || !sensors_out) return fail(UVRT_ERR_INVALID, "uvrt_read_sensors: null argument");
    if (c->sensor_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_read_sensors: no sensors (uvrt_set_sensors)");
    memcpy(sensors_out, c->sensors.data(), (size_t)c->sensor_count * sizeof(uvrt_sensor));
    return UVRT_OK;
}

int uvrt_drop_sensors(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_drop_sensors: null context");
    if (c->sensor_count <= 0) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->sensors_dev.release();
    c->sensor_planes.release();
    c->sensor_out.release();
    c->sensors.clear();
    c->sensor_count = 0;
    return UVRT_OK;
}

int uvrt_gather_sensors(uvrt_ctx* c, const uvrt_gather_params* prm, int32_t first, int32_t count)
{
    const char* who = "uvrt_gather_sensors";
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    const int32_t S = prm->samples;
    if (S < 1 || S > 4096) return fail(UVRT_ERR_INVALID, "%s: samples = %d must be in [1, 4096]", who, S);
    if (int rc = check_sensor_trace(c, first, count, S, who)) return rc;
    if (prm->photons_equiv <= 0) return fail(UVRT_ERR_INVALID, "%s: photons_equiv must be > 0", who);
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return fail(UVRT_ERR_INVALID, "%s: reserved fields must be 0", who);
    if (int rc = set_device(c)) return rc;
    if (int rc = begin_shadow_launch(c)) return rc;
    if (int rc = c->g_w.ensure((size_t)c->capacity * 8, false, c->stream)) return rc;
    SensorGenParams g;
    memset(&g, 0, sizeof g);
    g.sensors = c->sensors_dev.as<float4>();
    g.rays = c->lanes[0].rays.as<float4>();
    g.oxz = c->g_oxz.as<float2>();
    g.tmax = c->g_tmax.as<float>();
    g.w = c->g_w.as<double>();
    g.fx = prm->from[0]; g.fy = prm->from[1]; g.fz = prm->from[2];
    g.tx = prm->to[0]; g.ty = prm->to[1]; g.tz = prm->to[2];
    g.light_length = prm->light_length;
    g.seed_hash = host_wang_hash(prm->seed);
    g.samples = S;
    g.seed = prm->seed;
    g.mode = c->gather_sampling;
    SensorReduceParams r;
    memset(&r, 0, sizeof r);
    r.w = g.w;
    r.occluded = c->g_occ.as<uint8_t>();
    r.density = sensor_plane(c, 0);
    r.variance = sensor_plane(c, 1);
    r.samples = S;
    r.photons_equiv = prm->photons_equiv;
    r.mode = g.mode;
    return for_tri_chunks(c, S, count, [&](int32_t done, int32_t cnt) -> int {
        g.first = r.first = first + done;
        g.count = r.count = cnt;
        launch_sensor_generate(g, c->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = trace_shadow_rays(c, (int64_t)cnt * S, who)) return rc;
        launch_sensor_reduce(r, c->stream);
        HIP_TRY(hipGetLastError());
        return UVRT_OK;
    });
}

int uvrt_gather_sensors_indirect(uvrt_ctx* c, const uvrt_sensor_indirect_params* prm, int32_t first, int32_t count)
{
    const char* who = "uvrt_gather_sensors_indirect";
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    const int32_t S = prm->samples;
    if (S < 2 || S > 4096 || (S & 1)) return fail(UVRT_ERR_INVALID, "%s: samples = %d must be even and in [2, 4096]", who, S);
    if (int rc = check_sensor_trace(c, first, count, S, who)) return rc;
    if (!std::isfinite(prm->reflectance) || !(prm->reflectance >= 0.0f) || !(prm->reflectance <= 1.0f))
        return fail(UVRT_ERR_INVALID, "%s: reflectance must be finite and in [0, 1]", who);
    if (prm->emitter != 0 && prm->emitter != 1) return fail(UVRT_ERR_INVALID, "%s: emitter must be 0 or 1, not %d", who, prm->emitter);
    if (prm->use_map != 0 && prm->use_map != 1) return fail(UVRT_ERR_INVALID, "%s: use_map must be 0 or 1, not %d", who, prm->use_map);
    if (prm->use_map && prm->emitter != 1) return fail(UVRT_ERR_INVALID, "%s: use_map needs emitter 1 (the face planes)", who);
    if (prm->use_map && !c->derived.have_rho)
        return fail(UVRT_ERR_INVALID, "%s: no reflectance planes (uvrt_fill_reflectance / uvrt_write_reflectance)", who);
    if (prm->reserved != 0) return fail(UVRT_ERR_INVALID, "%s: reserved must be 0", who);
    if (int rc = set_device(c)) return rc;
    if (int rc = begin_closest_launch(c)) return rc;
    if (int rc = prm->emitter == 0 ? ensure_source(c) : ensure_faces(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    SensorGenParams g;
    memset(&g, 0, sizeof g);
    g.sensors = c->sensors_dev.as<float4>();
    g.rays = c->lanes[0].rays.as<float4>();
    g.oxz = c->g_oxz.as<float2>();
    g.tmax = c->g_tmax.as<float>();
    g.seed_hash = host_wang_hash(prm->seed);
    g.samples = S;
    g.seed = prm->seed;
    SensorIndirectReduceParams r;
    memset(&r, 0, sizeof r);
    r.sensors = g.sensors;
    r.gtris = c->derived.g_tris.as<float4>();
    r.rays = g.rays;
    r.hit = c->g_hit.as<uint2>();
    r.source = c->derived.source.as<double>();
    r.faces = c->derived.faces.as<double>();
    r.rho = prm->use_map ? c->derived.rho.as<float>() : nullptr;
    r.density = sensor_plane(c, 0);
    r.samples = S;
    r.T = c->T;
    r.reflectance = prm->reflectance;
    r.emitter = prm->emitter;
    r.use_map = prm->use_map;
    return for_tri_chunks(c, S, count, [&](int32_t done, int32_t cnt) -> int {
        g.first = r.first = first + done;
        g.count = r.count = cnt;
        launch_sensor_indirect_generate(g, c->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = trace_closest_rays(c, (int64_t)cnt * S, who)) return rc;
        launch_sensor_indirect_reduce(r, c->stream);
        HIP_TRY(hipGetLastError());
        return UVRT_OK;
    });
}

int uvrt_accumulate_sensors(uvrt_ctx* c, float time_step)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_accumulate_sensors: null context");
    if (c->sensor_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_accumulate_sensors: no sensors (uvrt_set_sensors)");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    launch_sensor_accumulate(c->sensor_planes.as<double>(), c->sensor_count, time_step, c->stream);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

int uvrt_reset_sensors(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_reset_sensors: null context");
    if (c->sensor_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_reset_sensors: no sensors (uvrt_set_sensors)");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipMemsetAsync(c->sensor_planes.p, 0, (size_t)c->sensor_count * 8 * kSensorPlanes, c->stream));
    return UVRT_OK;
}

int uvrt_read_sensor_plane(uvrt_ctx* c, int32_t which, double* out, int32_t first, int32_t count)
{
    return sensor_plane_range(c, "uvrt_read_sensor_plane", which, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_write_sensor_plane(uvrt_ctx* c, int32_t which, const double* in, int32_t first, int32_t count)
{
    return sensor_plane_range(c, "uvrt_write_sensor_plane", which, const_cast<double*>(in), first, count, hipMemcpyHostToDevice);
}

int uvrt_sensor_dosage(uvrt_ctx* c, int32_t which, int32_t photons_per_light, float scaled_power, float* out, int32_t first,
                       int32_t count)
{
    const char* who = "uvrt_sensor_dosage";
    if (!c || !out) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (c->sensor_count <= 0) return fail(UVRT_ERR_INVALID, "%s: no sensors (uvrt_set_sensors)", who);
    if (which != UVRT_MAP_SUM && which != UVRT_MAP_MAX) return fail(UVRT_ERR_INVALID, "%s: which_map must be 0 or 1", who);
    if (!range_ok(out, first, count, c->sensor_count))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->sensor_count);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    launch_sensor_dosage(sensor_plane(c, which == UVRT_MAP_SUM ? 2 : 3), c->sensor_out.as<float>(), photons_per_light, scaled_power,
                         first, count, c->stream);
    HIP_TRY(hipGetLastError());
    if (count == 0) { HIP_TRY(hipStreamSynchronize(c->stream)); return UVRT_OK; }
    return copy_sync(c, out, c->sensor_out.p, (size_t)count * 4, hipMemcpyDeviceToHost);
}

}  // extern "C"

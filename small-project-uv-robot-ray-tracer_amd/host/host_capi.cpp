// host_capi.cpp -- flat C wrappers over Mesh / BVH / RayTracer so that tests and bench.py can
// drive the C++ host layer through ctypes.  Plumbing only; no arithmetic lives here.
#include "raytracer.h"

#include <algorithm>
#include <cstddef>
#include <cstring>
#include <string>
#include <vector>

using namespace Tmpl8;

namespace {

// a route file's name as SaveRoute / LoadRoute take it: at most 31 characters
void copy_name(char out[32], const char* name)
{
    strncpy(out, name, 31);
    out[31] = 0;
}

std::vector<LightPos> positions(const float* xyd, int n)
{
    std::vector<LightPos> out;
    for (int i = 0; i < n; ++i) out.push_back({make_float2(xyd[3 * i], xyd[3 * i + 1]), xyd[3 * i + 2]});
    return out;
}

std::vector<RayTracer*> group(void** rs, int n) { return std::vector<RayTracer*>((RayTracer**)rs, (RayTracer**)rs + n); }

// a message for a ctypes caller: copied into err (cut to fit), 0 when it is empty and -1 otherwise
int report(const std::string& e, char* err, int err_len)
{
    if (err && err_len > 0) { strncpy(err, e.c_str(), (size_t)err_len - 1); err[err_len - 1] = 0; }
    return e.empty() ? 0 : -1;
}

}  // namespace

extern "C" {

// ---- Mesh ----
void* uvrt_host_mesh_load(const char* glb_path)
{
    Mesh* m = new Mesh();
    if (!m->LoadMeshFromFile(glb_path)) { delete m; return nullptr; }
    return m;
}
void* uvrt_host_mesh_from_tris(const void* tris64, int count)
{
    Mesh* m = new Mesh();
    m->SetTriangles((const Tri*)tris64, count);
    return m;
}
void uvrt_host_mesh_free(void* m) { delete (Mesh*)m; }
int uvrt_host_mesh_tri_count(void* m) { return ((Mesh*)m)->triangleCount; }
float uvrt_host_mesh_floor_height(void* m) { return ((Mesh*)m)->floorHeight; }
const void* uvrt_host_mesh_tris(void* m) { return ((Mesh*)m)->triangles; }
const void* uvrt_host_mesh_nodes(void* m) { return ((Mesh*)m)->bvh->bvhNode; }
unsigned uvrt_host_mesh_nodes_used(void* m) { return ((Mesh*)m)->bvh->nodesUsed; }
const unsigned* uvrt_host_mesh_tri_idx(void* m) { return ((Mesh*)m)->bvh->triIdx; }
void uvrt_host_mesh_rebuild_bvh(void* m) { ((Mesh*)m)->bvh->Build(); }

// ---- RayTracer ----
void* uvrt_host_rt_new(void) { return new RayTracer(); }
void uvrt_host_rt_free(void* r) { delete (RayTracer*)r; }
void uvrt_host_rt_set_route_dir(void* r, const char* dir) { ((RayTracer*)r)->routeDir = dir; }
void uvrt_host_rt_set_default_route(void* r, const char* name)
{ copy_name(((RayTracer*)r)->defaultRouteFile, name); }
void uvrt_host_rt_set_device(void* r, int dev) { ((RayTracer*)r)->deviceId = dev; }
void uvrt_host_rt_set_auto_save(void* r, int on) { ((RayTracer*)r)->autoSaveRoute = on != 0; }
void uvrt_host_rt_init(void* r, void* mesh) { ((RayTracer*)r)->Init((Mesh*)mesh); }
void uvrt_host_rt_load_route(void* r, const char* name)
{
    char buf[32];
    copy_name(buf, name);
    ((RayTracer*)r)->LoadRoute(buf);
}
void uvrt_host_rt_save_route(void* r, const char* name)
{
    char buf[32];
    copy_name(buf, name);
    ((RayTracer*)r)->SaveRoute(buf);
}
void uvrt_host_rt_update_photons_per_light(void* r) { ((RayTracer*)r)->UpdatePhotonsPerLight(); }
void uvrt_host_rt_reset_dosage_map(void* r) { ((RayTracer*)r)->ResetDosageMap(); }
void uvrt_host_rt_clear_buffers(void* r, int reset_color) { ((RayTracer*)r)->ClearBuffers(reset_color != 0); }
void uvrt_host_rt_compute_dosage_map(void* r) { ((RayTracer*)r)->ComputeDosageMap(); }
void uvrt_host_rt_compute_single(void* r, float x, float y, float duration, int photons, int tris)
{
    ((RayTracer*)r)->ComputeSingleLightDosageMap({make_float2(x, y), duration}, photons, tris);
}
void uvrt_host_rt_compute_segment(void* r, float ax, float ay, float bx, float by, int photons, int tris)
{
    ((RayTracer*)r)->ComputeSegmentDosageMap({make_float2(ax, ay), 0.0f}, {make_float2(bx, by), 0.0f}, photons, tris);
}
void uvrt_host_rt_compute_segments(void* r) { ((RayTracer*)r)->ComputeSegments(); }
void uvrt_host_rt_shade(void* r) { ((RayTracer*)r)->Shade(); }
void uvrt_host_rt_add_lamp(void* r) { ((RayTracer*)r)->AddLamp(); }
void uvrt_host_rt_calibrate(void* r, float p, float h, float d) { ((RayTracer*)r)->CalibratePower(p, h, d); }
void uvrt_host_rt_sync(void* r) { ((RayTracer*)r)->Sync(); }
void uvrt_host_rt_read_dosage(void* r, float* out, int first, int count) { ((RayTracer*)r)->ReadDosage(out, first, count); }
void* uvrt_host_rt_ctx(void* r) { return ((RayTracer*)r)->ctx; }
void uvrt_host_rt_set_shard(void* r, int rank, int world)
{
    ((RayTracer*)r)->shardRank = rank;
    ((RayTracer*)r)->shardWorld = world;
    ((RayTracer*)r)->launchIndex = 0;
}

// RayTracer::reflectMap (the rules file; "" for none) and the caller's planes (SetReflectanceMap; count 0 forgets them);
// uvrt_host_rt_reflectance_map returns the size of the active map (ActiveReflectanceMap) and copies at most n values;
// uvrt_host_rt_prepare_reflect_map is PrepareReflectMap: 0, or -1 and the message in err
void uvrt_host_rt_set_reflect_map(void* r, const char* file) { ((RayTracer*)r)->reflectMap = file ? file : ""; }
int uvrt_host_rt_get_reflect_map(void* r, char* out, int n)
{
    const std::string& f = ((RayTracer*)r)->reflectMap;
    if (n > 0) { strncpy(out, f.c_str(), (size_t)n - 1); out[n - 1] = 0; }
    return (int)f.size();
}
void uvrt_host_rt_set_reflectance_map(void* r, const float* rho2T, int count) { ((RayTracer*)r)->SetReflectanceMap(rho2T, count); }
int uvrt_host_rt_reflectance_map(void* r, float* out, int n)
{
    const std::vector<float>& v = ((RayTracer*)r)->ActiveReflectanceMap();
    for (int i = 0; i < n && i < (int)v.size(); ++i) out[i] = v[i];
    return (int)v.size();
}
int uvrt_host_rt_has_reflect_map(void* r) { return ((RayTracer*)r)->HasReflectanceMap() ? 1 : 0; }
int uvrt_host_rt_prepare_reflect_map(void* r, float base, char* err, int err_len)
{
    return report(((RayTracer*)r)->PrepareReflectMap(base), err, err_len);
}
// RayTracer::ParseReflectRules over `count` 64-byte Tri records: 0 and out[2 * count], or -1 and the message in err
int uvrt_host_reflect_rules(const char* path, const void* tris64, int count, float base, float* out, char* err, int err_len)
{
    return report(RayTracer::ParseReflectRules(path, (const Tri*)tris64, count, base, out), err, err_len);
}

// RayTracer::mirrorMap (the rules file; "" for none) and the caller's panels (SetMirrors; count 0 forgets them);
// uvrt_host_rt_prepare_mirror_map is PrepareMirrorMap: 0, or -1 and the message in err
void uvrt_host_rt_set_mirror_map(void* r, const char* file) { ((RayTracer*)r)->mirrorMap = file ? file : ""; }
int uvrt_host_rt_get_mirror_map(void* r, char* out, int n)
{
    const std::string& f = ((RayTracer*)r)->mirrorMap;
    if (n > 0) { strncpy(out, f.c_str(), (size_t)n - 1); out[n - 1] = 0; }
    return (int)f.size();
}
void uvrt_host_rt_set_mirrors(void* r, const uvrt_mirror* panels, int count, const unsigned char* panel_of_tri, int n_tris)
{
    ((RayTracer*)r)->SetMirrors(panels, count, panel_of_tri, n_tris);
}
int uvrt_host_rt_has_mirrors(void* r) { return ((RayTracer*)r)->HasMirrors() ? 1 : 0; }
int uvrt_host_rt_prepare_mirror_map(void* r, char* err, int err_len)
{
    return report(((RayTracer*)r)->PrepareMirrorMap(), err, err_len);
}
// RayTracer::ParseMirrorRules over `count` 64-byte Tri records: 0, *panels_count, panels_out[8] and panel_of_tri_out[count], or
// -1 and the message in err
int uvrt_host_mirror_rules(const char* path, const void* tris64, int count, uvrt_mirror* panels_out, int* panels_count,
                           unsigned char* panel_of_tri_out, char* err, int err_len)
{
    return report(RayTracer::ParseMirrorRules(path, (const Tri*)tris64, count, panels_out, panels_count, panel_of_tri_out), err, err_len);
}

// RayTracer::sensorMap (the rules file; "" for none) and the caller's sensors (SetSensors; count 0 forgets them);
// uvrt_host_rt_prepare_sensor_map is PrepareSensorMap: 0, or -1 and the message in err; uvrt_host_rt_active_sensors returns the
// number of active sensors (ActiveSensors) and copies at most n records
void uvrt_host_rt_set_sensor_map(void* r, const char* file) { ((RayTracer*)r)->sensorMap = file ? file : ""; }
int uvrt_host_rt_get_sensor_map(void* r, char* out, int n)
{
    const std::string& f = ((RayTracer*)r)->sensorMap;
    if (n > 0) { strncpy(out, f.c_str(), (size_t)n - 1); out[n - 1] = 0; }
    return (int)f.size();
}
void uvrt_host_rt_set_sensors(void* r, const uvrt_sensor* sensors, int count)
{
    ((RayTracer*)r)->SetSensors(std::vector<uvrt_sensor>(sensors, sensors + std::max(count, 0)));
}
int uvrt_host_rt_has_sensors(void* r) { return ((RayTracer*)r)->HasSensors() ? 1 : 0; }
int uvrt_host_rt_prepare_sensor_map(void* r, char* err, int err_len)
{
    return report(((RayTracer*)r)->PrepareSensorMap(), err, err_len);
}
int uvrt_host_rt_active_sensors(void* r, uvrt_sensor* out, int n)
{
    const std::vector<uvrt_sensor>& v = ((RayTracer*)r)->ActiveSensors();
    for (int i = 0; i < n && i < (int)v.size(); ++i) out[i] = v[i];
    return (int)v.size();
}
// RayTracer::ReadSensors: returns the number of sensors and copies at most n entries of each
int uvrt_host_rt_read_sensors(void* r, float* dose, float* peak, double* std_err, int n)
{
    std::vector<float> d, p;
    std::vector<double> e;
    ((RayTracer*)r)->ReadSensors(d, p, e);
    for (int i = 0; i < n && i < (int)d.size(); ++i) { dose[i] = d[i]; peak[i] = p[i]; std_err[i] = e[i]; }
    return (int)d.size();
}
void uvrt_host_rt_calibrate_at_sensor(void* r, float p, int sensor, int light) { ((RayTracer*)r)->CalibratePowerAtSensor(p, sensor, light); }
// RayTracer::ParseSensorRules: 0, *count and at most `max` records in out, or -1 and the message in err
int uvrt_host_sensor_rules(const char* path, uvrt_sensor* out, int max, int* count, char* err, int err_len)
{
    std::vector<uvrt_sensor> v;
    const std::string e = RayTracer::ParseSensorRules(path, &v);
    if (e.empty()) {
        *count = (int)v.size();
        for (int i = 0; i < max && i < (int)v.size(); ++i) out[i] = v[i];
    }
    return report(e, err, err_len);
}

// RayTracer::gatherRelError and gatherMaxExtra (the adaptive gather of every gather launch; rel_error 0: off)
void uvrt_host_rt_set_gather_refine(void* r, double rel_error, int max_extra)
{
    ((RayTracer*)r)->gatherRelError = rel_error;
    ((RayTracer*)r)->gatherMaxExtra = max_extra;
}

void uvrt_host_rt_compute_batched(void* r, int iterations) { ((RayTracer*)r)->ComputeIterationsBatched(iterations); }
void uvrt_host_rt_compute_batched_group(void** rs, int n, int iterations)
{
    RayTracer::ComputeIterationsBatched(group(rs, n), iterations);
}
void uvrt_host_rt_set_ray_range(void* r, int rank, int world) { ((RayTracer*)r)->SetRayRange(rank, world); }
void uvrt_host_rt_set_reduce_over_comm(void* r, int on) { ((RayTracer*)r)->reduceOverComm = on != 0; }

int uvrt_host_rt_lamp_count(void* r) { return (int)((RayTracer*)r)->lightPositions.size(); }
void uvrt_host_rt_get_lamp(void* r, int i, float* xyd)
{
    const LightPos& lp = ((RayTracer*)r)->lightPositions[i];
    xyd[0] = lp.position.x; xyd[1] = lp.position.y; xyd[2] = lp.duration;
}
void uvrt_host_rt_set_lamps(void* r, const float* xyd, int n)
{
    RayTracer* rt = (RayTracer*)r;
    rt->lightPositions = positions(xyd, n);
    rt->UpdatePhotonsPerLight();
}
// RayTracer::RouteLaunches of L positions (x, z, duration): returns the count, writes at most `max` 40-byte RouteLaunch records
int uvrt_host_route_launches(const float* xzd, int L, float y, float drive_speed, void* out, int max)
{
    static_assert(sizeof(RouteLaunch) == 40, "the record host.ROUTE_LAUNCH_DT describes");
    const std::vector<RouteLaunch> list = RayTracer::RouteLaunches(positions(xzd, L), y, drive_speed);
    const size_t n = std::min(list.size(), (size_t)std::max(max, 0));
    if (n) memcpy(out, list.data(), n * sizeof(RouteLaunch));
    return (int)list.size();
}

// duration planning: RayTracer::PlanOptions as one plain struct (host.PlanOptions mirrors it field for field; a new option is
// a line in X below and one there).  uvrt_host_plan_options_init writes the defaults of RayTracer::PlanOptions{};
// uvrt_host_plan_options_layout writes every field's offset in declaration order, then the size, and returns how many numbers
// that is (at most `max` are written): the mirror is held to it.
#define UVRT_HOST_PLAN_OPTIONS(X) \
    X(float, min_dose, minDose) X(int, min_photons, minPhotons) X(double, margin, margin) X(double, rel_gap, relGap) \
    X(int, max_iterations, maxIterations) X(const unsigned char*, mask, mask) X(int, gather_samples, gatherSamples) \
    X(int, gather_sampling, gatherSampling) X(double, gather_confidence, gatherConfidence) \
    X(double, gather_rel_error, gatherRelError) X(int, gather_max_extra, gatherMaxExtra) X(float, reflectance, reflectance) \
    X(int, reflect_samples, reflectSamples) X(int, reflect_bounces, reflectBounces) X(int, reflect_sided, reflectSided) \
    X(int, reflect_mapped, reflectMapped) X(int, mirror_mapped, mirrorMapped) X(int, gather_batch, gatherBatch)
struct uvrt_host_plan_options {
#define X(type, name, member) type name;
    UVRT_HOST_PLAN_OPTIONS(X)
#undef X
};
static RayTracer::PlanOptions plan_options(const uvrt_host_plan_options* o)
{
    RayTracer::PlanOptions p;
#define X(type, name, member) p.member = o->name;
    UVRT_HOST_PLAN_OPTIONS(X)
#undef X
    return p;
}
void uvrt_host_plan_options_init(uvrt_host_plan_options* o)
{
    const RayTracer::PlanOptions p;
#define X(type, name, member) o->name = p.member;
    UVRT_HOST_PLAN_OPTIONS(X)
#undef X
}
int uvrt_host_plan_options_layout(int* out, int max)
{
    const int layout[] = {
#define X(type, name, member) (int)offsetof(uvrt_host_plan_options, name),
        UVRT_HOST_PLAN_OPTIONS(X)
#undef X
        (int)sizeof(uvrt_host_plan_options)};
    const int n = (int)(sizeof layout / sizeof layout[0]);
    for (int i = 0; i < n && i < max; ++i) out[i] = layout[i];
    return n;
}
// durations -> lightPositions, report -> *rep, starting SEED -> *seed
void uvrt_host_rt_plan(void* r, const uvrt_host_plan_options* o, uvrt_plan_report* rep, unsigned* seed)
{
    *rep = ((RayTracer*)r)->PlanDurations(plan_options(o), seed);
}
void uvrt_host_rt_plan_group(void** rs, int n, const uvrt_host_plan_options* o, uvrt_plan_report* rep, unsigned* seed)
{
    *rep = RayTracer::PlanDurations(group(rs, n), plan_options(o), seed);
}
// of the last PlanDurations: the bounds report and the segment columns (returns their number; copies at most n)
void uvrt_host_rt_plan_bounds(void* r, uvrt_plan_bounds_report* out) { *out = ((RayTracer*)r)->planBounds; }
int uvrt_host_rt_plan_segments(void* r, float* out, int n)
{
    const std::vector<float>& s = ((RayTracer*)r)->planSegmentDurations;
    for (int i = 0; i < n && i < (int)s.size(); ++i) out[i] = s[i];
    return (int)s.size();
}
void uvrt_host_rt_end_plan(void* r) { ((RayTracer*)r)->EndPlan(); }
void uvrt_host_rt_set_candidate_grid(void* r, int nx, int nz, float inset) { ((RayTracer*)r)->SetCandidateGrid(nx, nz, inset); }
void uvrt_host_grid_positions(float xmin, float xmax, float zmin, float zmax, int nx, int nz, float inset, float* xz)
{
    RayTracer::GridPositions(xmin, xmax, zmin, zmax, nx, nz, inset, xz);
}

// scalar fields, by name (keeps the ctypes surface small)
static int field(RayTracer* rt, const char* n, double* v, int set)
{
#define F(name, type) if (!strcmp(n, #name)) { if (set) rt->name = (type)*v; else *v = (double)rt->name; return 0; }
    F(lightLength, float) F(lightHeight, float) F(maxPhotonCount, int) F(photonCount, int)
    F(maxIterations, int) F(currIterations, int) F(lightIntensity, float) F(minDosage, float)
    F(minPower, float) F(photonsPerLight, int) F(compTime, float) F(progress, float)
    F(finishedComputation, bool) F(thresholdView, bool) F(startedComputation, bool)
    F(calibratedPower, float) F(photonMapSize, int) F(driveSpeed, float) F(gatherSamples, int)
    F(gatherSampling, int) F(gatherRelError, double) F(gatherMaxExtra, int)
    F(reflectance, float) F(reflectSamples, int) F(reflectBounces, int) F(gatherBatch, int)
    F(reflectSided, int) F(sensorSamples, int) F(sensorLaunches, unsigned)
#undef F
    if (!strcmp(n, "viewMode")) { if (set) rt->viewMode = (ViewMode)(int)*v; else *v = (double)rt->viewMode; return 0; }
    return -1;
}
int uvrt_host_rt_get(void* r, const char* name, double* v) { return field((RayTracer*)r, name, v, 0); }
int uvrt_host_rt_set(void* r, const char* name, double v) { return field((RayTracer*)r, name, &v, 1); }

}  // extern "C"

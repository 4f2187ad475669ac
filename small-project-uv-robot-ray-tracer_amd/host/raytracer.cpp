// raytracer.cpp -- host orchestration of the UV-dose hot path on the HIP C ABI
// (reference: raytracer.cpp:3-300; launch sequence in SURVEY.md 3.2).
//
// Same call order as the reference: per lamp generate -> extend -> accumulate on one in-order
// stream with no host synchronisation in between; Shade = computeDosage + dosageToColor;
// errors of the device layer are fatal (the reference's CHECKCL -> FatalError, exit).
#include "raytracer.h"
#include "raytracer_internal.h"

#include "../../include/uvrt.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <sstream>

using namespace Tmpl8;
using namespace Tmpl8::host_internal;

namespace {

// ------------------------------------------------------------ minimal XML for route files
struct XmlElem {
    std::string name, text;
    std::vector<std::pair<std::string, std::string>> attrs;
    std::vector<XmlElem> kids;
    const XmlElem* child(const std::string& n) const
    {
        for (auto& k : kids) if (k.name == n) return &k;
        return nullptr;
    }
    const std::string* attr(const std::string& n) const
    {
        for (auto& a : attrs) if (a.first == n) return &a.second;
        return nullptr;
    }
};

struct XmlParser {
    const std::string& s;
    size_t i = 0;
    bool ok = true;
    explicit XmlParser(const std::string& str) : s(str) {}
    void ws() { while (i < s.size() && isspace((unsigned char)s[i])) ++i; }
    std::string ident()
    {
        size_t b = i;
        while (i < s.size() && (isalnum((unsigned char)s[i]) || s[i] == '_' || s[i] == '-' || s[i] == ':' || s[i] == '.')) ++i;
        return s.substr(b, i - b);
    }
    void skip_misc()
    {
        for (;;) {
            ws();
            if (s.compare(i, 4, "<!--") == 0) { size_t e = s.find("-->", i); i = e == std::string::npos ? s.size() : e + 3; }
            else if (s.compare(i, 2, "<?") == 0) { size_t e = s.find("?>", i); i = e == std::string::npos ? s.size() : e + 2; }
            else break;
        }
    }
    bool element(XmlElem& out)
    {
        skip_misc();
        if (i >= s.size() || s[i] != '<') return ok = false;
        ++i;
        out.name = ident();
        for (;;) {
            ws();
            if (i >= s.size()) return ok = false;
            if (s[i] == '/') { i += 2; return true; }            // <name ... />
            if (s[i] == '>') { ++i; break; }
            std::string an = ident();
            ws();
            if (an.empty() || i >= s.size() || s[i] != '=') return ok = false;
            ++i;
            ws();
            if (i >= s.size() || (s[i] != '"' && s[i] != '\'')) return ok = false;
            const char q = s[i++];
            size_t e = s.find(q, i);
            if (e == std::string::npos) return ok = false;
            out.attrs.emplace_back(an, s.substr(i, e - i));
            i = e + 1;
        }
        for (;;) {                                               // content
            size_t lt = s.find('<', i);
            if (lt == std::string::npos) return ok = false;
            out.text += s.substr(i, lt - i);
            i = lt;
            if (s.compare(i, 2, "</") == 0) {
                size_t e = s.find('>', i);
                if (e == std::string::npos) return ok = false;
                i = e + 1;
                return true;
            }
            if (s.compare(i, 4, "<!--") == 0) { skip_misc(); continue; }
            XmlElem kid;
            if (!element(kid)) return false;
            out.kids.push_back(std::move(kid));
        }
    }
};

std::string trim(const std::string& t)
{
    size_t b = 0, e = t.size();
    while (b < e && isspace((unsigned char)t[b])) ++b;
    while (e > b && isspace((unsigned char)t[e - 1])) --e;
    return t.substr(b, e - b);
}
// tinyxml2 XMLUtil::ToInt / ToFloat: sscanf "%d" / "%f"
bool to_int(const std::string& t, int* v) { return sscanf(t.c_str(), "%d", v) == 1; }
bool to_float(const std::string& t, float* v) { return sscanf(t.c_str(), "%f", v) == 1; }
// tinyxml2 XMLUtil::ToStr(float): "%.8g"
std::string float_str(float v) { char b[64]; snprintf(b, sizeof b, "%.8g", (double)v); return b; }

// A 0/1 state of the context that a launch needs on: read, set to 1, and put back when the scope ends (nothing when not armed)
struct ContextState {
    int (*get)(uvrt_ctx*, int32_t*);
    int (*set)(uvrt_ctx*, int32_t);
    const char *getName, *setName;
};
const ContextState kVariancePlane = {uvrt_get_gather_variance, uvrt_set_gather_variance, "get_gather_variance", "set_gather_variance"};
const ContextState kFacePlanes = {uvrt_get_gather_faces, uvrt_set_gather_faces, "get_gather_faces", "set_gather_faces"};
struct ScopedState {
    ScopedState(uvrt_ctx* c, const ContextState& s, bool on) : ctx(c), state(s), armed(on)
    {
        if (!armed) return;
        check(state.get(ctx, &before), state.getName);
        check(state.set(ctx, 1), state.setName);
    }
    ~ScopedState() { if (armed) check(state.set(ctx, before), state.setName); }
    ScopedState(const ScopedState&) = delete;
    ScopedState& operator=(const ScopedState&) = delete;
    uvrt_ctx* ctx;
    const ContextState& state;
    bool armed;
    int32_t before = 0;
};

}  // namespace

RayTracer::~RayTracer()
{
    if (ctx) uvrt_destroy(ctx);
    delete[] dosageMap;
}

void RayTracer::AddLamp()                                    // raytracer.cpp:3-10
{
    lightPositions.push_back({make_float2(0.0f, 0.0f), 1.0f});
    UpdatePhotonsPerLight();
}

void RayTracer::Init(Mesh* m)                                // raytracer.cpp:12-59
{
    mesh = m;
    LoadRoute(defaultRouteFile);
    // A second Init (model reload, userinterface.cpp:239-240) rebuilds the kernels in the
    // reference, which restarts SEED at 0; a fresh context does the same (and does not leak).
    if (ctx) { uvrt_destroy(ctx); ctx = nullptr; }
    check(uvrt_create(deviceId, &ctx), "uvrt_create");
    check(uvrt_set_scene(ctx, mesh->triangles, mesh->triangleCount, mesh->bvh->bvhNode,
                         (int)mesh->bvh->nodesUsed, mesh->bvh->triIdx), "uvrt_set_scene");
}

void RayTracer::UpdatePhotonsPerLight()                      // raytracer.cpp:61-64
{
    // Round down to an even number, as the reference does.  (An empty lamp list divides by
    // zero in the reference; kept as the caller's error.)
    if (lightPositions.empty()) { photonsPerLight = 0; return; }   // the reference divides by zero here
    photonsPerLight = (int)(photonCount / lightPositions.size()) & ~1;
}

std::vector<RouteLaunch> RayTracer::RouteLaunches(const std::vector<LightPos>& positions, float y, float driveSpeed)
{
    const size_t L = positions.size();
    std::vector<RouteLaunch> list;
    for (size_t i = 0; i < L; ++i) {                         // raytracer.cpp:77 -- the lamp's foot in world space
        const LightPos& p = positions[i];
        list.push_back({{p.position.x, y, p.position.y}, {0.0f, 0.0f, 0.0f}, p.duration, UVRT_LAUNCH_STOP, (int)i, 0});
    }
    if (!(driveSpeed > 0.0f) || L < 2) return list;
    for (size_t k = 0; k + 1 < L; ++k) {
        const LightPos &a = positions[k], &b = positions[k + 1];
        const float dx = b.position.x - a.position.x, dz = b.position.y - a.position.y;
        const float len = sqrtf(dx * dx + dz * dz);
        list.push_back({{a.position.x, y, a.position.y}, {b.position.x, y, b.position.y}, len / driveSpeed, UVRT_LAUNCH_SWEEP, (int)(L + k), 0});
    }
    return list;
}

std::vector<RouteLaunch> RayTracer::Launches() const
{
    return RouteLaunches(lightPositions, mesh->floorHeight + lightHeight, driveSpeed);   // the y sum is one f32 addition
}

void RayTracer::ComputeDosageMap()                           // raytracer.cpp:66-72
{
    RunLaunches(Launches(), photonsPerLight, mesh->triangleCount, OwnGather(), false);
}

// ------------------------------------------------------------ how a launch gathers (raytracer.h GatherOptions)
RayTracer::GatherOptions RayTracer::OwnGather() const
{
    GatherOptions g;
    g.samples = gatherSamples; g.sampling = gatherSampling;
    g.relError = gatherRelError; g.maxExtra = gatherMaxExtra;
    g.reflectance = reflectance; g.reflectSamples = reflectSamples; g.reflectBounces = reflectBounces;
    g.sided = reflectSided; g.mapped = HasReflectanceMap(); g.mirrored = HasMirrors();
    g.batch = gatherBatch;
    g.sensors = HasSensors();
    return g;
}

RayTracer::GatherOptions RayTracer::PlanGather(const PlanOptions& opt)
{
    GatherOptions g;
    g.samples = opt.gatherSamples; g.sampling = opt.gatherSampling;
    g.relError = opt.gatherRelError; g.maxExtra = opt.gatherMaxExtra;
    g.reflectance = opt.reflectance; g.reflectSamples = opt.reflectSamples; g.reflectBounces = opt.reflectBounces;
    g.sided = opt.reflectSided; g.mapped = opt.reflectMapped != 0; g.mirrored = opt.mirrorMapped != 0;
    g.batch = opt.gatherBatch;
    return g;
}

const char* RayTracer::GatherRefusal(const GatherOptions& g, int checks, bool plan)
{
    if (checks & kBatchRefusals) {
        if (g.batch < 0 || g.batch > UVRT_GATHER_BATCH_MAX) return "gatherBatch must be in [0, 64]";
        if (g.sided != 0 && g.batch >= 2) return "reflectSided is not supported with gatherBatch >= 2 (a gather batch keeps no face planes)";
    }
    if (!(checks & kLaunchRefusals)) return nullptr;
    if (g.reflectBounces < 0 || g.reflectBounces > 16) return "reflectBounces must be in [0, 16]";
    if (g.sided != 0) {
        if (g.sided != 1) return "reflectSided must be 0 or 1";
        if (g.reflectance == 0.0f) return "reflectSided needs reflectance > 0 (without a bounce there are no faces to resolve)";
        if (g.reflectBounces < 1) return "reflectSided needs reflectBounces >= 1 (the traced single bounce has no face-resolved form)";
    }
    if (g.mapped && g.sided == 0)
        return plan ? "reflectMapped needs reflectSided = 1 (only the face-resolved bounces know which face a reflectance belongs to)"
                    : "reflectMap needs reflectSided = 1 (only the face-resolved bounces know which face a reflectance belongs to)";
    if (g.relError != 0.0) {
        if (g.samples < 2)
            return plan ? "gatherRelError needs a plan from the direct gather with gatherSamples >= 2"
                        : "gatherRelError > 0 needs gatherSamples >= 2 (the refine reads the variance plane)";
        if (!(g.relError > 0.0) || !std::isfinite(g.relError)) return "gatherRelError must be finite and >= 0";
    }
    if (g.reflectance != 0.0f && g.samples < 1)
        return plan ? "reflectance needs a plan from the direct gather (gatherSamples > 0)"
                    : "reflectance > 0 needs gatherSamples > 0 (the bounce gathers over the direct gather's plane)";
    if (!(g.reflectance >= 0.0f) || !(g.reflectance <= 1.0f)) return "reflectance must be in [0, 1]";
    if (g.mirrored && g.samples < 1)
        return plan ? "mirrorMapped needs a plan from the direct gather (gatherSamples > 0)"
                    : "mirrorMap needs gatherSamples > 0 (the mirror gather adds to the direct gather's plane)";
    return nullptr;
}

// ------------------------------------------------------------ the reflectance map (raytracer.h reflectMap)
std::string RayTracer::ParseReflectRules(const char* path, const Tri* tris, int triangleCount, float base, float* out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return std::string(path) + ": cannot be read";
    const size_t T = (size_t)std::max(triangleCount, 0);
    for (size_t i = 0; i < 2 * T; ++i) out[i] = base;
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        auto bad = [&](const std::string& why) { return std::string(path) + ":" + std::to_string(no) + ": " + why; };
        std::istringstream ss(line.substr(0, line.find('#')));
        std::vector<std::string> w;
        for (std::string word; ss >> word;) w.push_back(word);
        if (w.empty()) continue;
        if (w[0] != "box") return bad("unknown keyword '" + w[0] + "'");
        const bool toward = w.size() == 12 && w[8] == "toward";
        if (w.size() != 8 && !toward) return bad("box takes X0 Y0 Z0 X1 Y1 Z1 RHO [toward PX PY PZ]");
        float v[7], p[3] = {0.0f, 0.0f, 0.0f};
        for (int k = 0; k < 7; ++k)
            if (!rule_number(w[1 + k], &v[k])) return bad("'" + w[1 + k] + "' is not a number");
        for (int k = 0; toward && k < 3; ++k)
            if (!rule_number(w[9 + k], &p[k]) || !std::isfinite(p[k])) return bad("'" + w[9 + k] + "' is not a finite number");
        const float rho = v[6];
        if (!std::isfinite(rho) || !(rho >= 0.0f) || !(rho <= 1.0f)) return bad("RHO must be finite and in [0, 1]");
        if (v[0] > v[3] || v[1] > v[4] || v[2] > v[5]) return bad("a lower bound of the box lies above its upper bound");
        for (size_t t = 0; t < T; ++t) {
            const Tri& tr = tris[t];
            const float3_strict& c = tr.centroid;
            if (!(c.x >= v[0] && c.x <= v[3] && c.y >= v[1] && c.y <= v[4] && c.z >= v[2] && c.z <= v[5])) continue;
            if (!toward) { out[t] = out[T + t] = rho; continue; }
            // the device's normal: the f32 edges, their cross product in f64 (uvrt_device.h tri_normal)
            const double ax = (double)(tr.vertex1.x - tr.vertex0.x), ay = (double)(tr.vertex1.y - tr.vertex0.y),
                         az = (double)(tr.vertex1.z - tr.vertex0.z);
            const double bx = (double)(tr.vertex2.x - tr.vertex0.x), by = (double)(tr.vertex2.y - tr.vertex0.y),
                         bz = (double)(tr.vertex2.z - tr.vertex0.z);
            const double nx = ay * bz - az * by, ny = az * bx - ax * bz, nz = ax * by - ay * bx;
            if (sqrt((nx * nx + ny * ny) + nz * nz) == 0.0) continue;
            const double dx = (double)p[0] - (double)tr.vertex0.x, dy = (double)p[1] - (double)tr.vertex0.y,
                         dz = (double)p[2] - (double)tr.vertex0.z;
            const double d = (nx * dx + ny * dy) + nz * dz;
            out[(d > 0.0 ? 0 : T) + t] = rho;
        }
    }
    return std::string();
}

void RayTracer::SetReflectanceMap(const float* rho2T, int count)
{
    if (count < 0 || (count > 0 && !rho2T)) fatal("SetReflectanceMap: no values");
    reflectMapValues.assign(rho2T, rho2T + count);
    reflectValuesStamp = reflectStampNext++;
}

std::string RayTracer::ReflectMapPath() const
{
    return reflectMap.empty() || reflectMap[0] == '/' ? reflectMap : routeDir + reflectMap;
}

std::string RayTracer::PrepareReflectMap(float base)
{
    if (reflectMap.empty()) return std::string();
    if (!mesh) return "reflectMap: no mesh (Init comes first)";
    const std::string path = ReflectMapPath();
    const size_t n = 2 * (size_t)mesh->triangleCount;
    if (reflectFileParsed == path && memcmp(&reflectFileBase, &base, 4) == 0 && reflectFileValues.size() == n) return std::string();
    reflectFileParsed.clear();
    reflectFileValues.assign(n, 0.0f);
    const std::string err = ParseReflectRules(path.c_str(), mesh->triangles, mesh->triangleCount, base, reflectFileValues.data());
    if (!err.empty()) { reflectFileValues.clear(); return err; }
    reflectFileParsed = path;
    reflectFileBase = base;
    reflectFileStamp = reflectStampNext++;
    return std::string();
}

const std::vector<float>& RayTracer::ActiveReflectanceMap() const
{
    static const std::vector<float> none;
    if (reflectMap.empty()) return reflectMapValues;
    return reflectFileParsed == ReflectMapPath() ? reflectFileValues : none;
}

void RayTracer::UploadReflectanceMap(int triangleCount, float base)
{
    const std::string err = PrepareReflectMap(base);
    if (!err.empty()) fatal(("reflectMap: " + err).c_str());
    const std::vector<float>& values = ActiveReflectanceMap();
    const unsigned long long stamp = reflectMap.empty() ? reflectValuesStamp : reflectFileStamp;
    if (values.size() != 2 * (size_t)triangleCount) fatal("the reflectance map must hold 2 x triangleCount values");
    int32_t have = 0;
    check(uvrt_reflectance_info(ctx, &have), "reflectance_info");
    if (have && reflectUploaded == stamp) return;
    for (int f = 0; f < 2; ++f)
        check(uvrt_write_reflectance(ctx, f, values.data() + (size_t)f * (size_t)triangleCount, 0, triangleCount), "write_reflectance");
    reflectUploaded = stamp;
}

// ------------------------------------------------------------ specular panels (raytracer.h mirrorMap)
std::string RayTracer::ParseMirrorRules(const char* path, const Tri* tris, int triangleCount, uvrt_mirror* panelsOut, int* countOut,
                                        uint8_t* panelOfTriOut)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return std::string(path) + ": cannot be read";
    const size_t T = (size_t)std::max(triangleCount, 0);
    for (size_t t = 0; t < T; ++t) panelOfTriOut[t] = 0;
    int count = 0;
    *countOut = 0;
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        auto bad = [&](const std::string& why) { return std::string(path) + ":" + std::to_string(no) + ": " + why; };
        std::istringstream ss(line.substr(0, line.find('#')));
        std::vector<std::string> w;
        for (std::string word; ss >> word;) w.push_back(word);
        if (w.empty()) continue;
        if (w[0] != "mirror") return bad("unknown keyword '" + w[0] + "'");
        if (w.size() != 15 || w[8] != "plane") return bad("mirror takes X0 Y0 Z0 X1 Y1 Z1 RHO plane QX QY QZ MX MY MZ");
        float v[7], q[6];
        for (int k = 0; k < 7; ++k)
            if (!rule_number(w[1 + k], &v[k])) return bad("'" + w[1 + k] + "' is not a number");
        for (int k = 0; k < 6; ++k)
            if (!rule_number(w[9 + k], &q[k]) || !std::isfinite(q[k])) return bad("'" + w[9 + k] + "' is not a finite number");
        const float rho = v[6];
        if (!std::isfinite(rho) || !(rho >= 0.0f) || !(rho <= 1.0f)) return bad("RHO must be finite and in [0, 1]");
        if (q[3] == 0.0f && q[4] == 0.0f && q[5] == 0.0f) return bad("the plane's normal is zero");
        if (v[0] > v[3] || v[1] > v[4] || v[2] > v[5]) return bad("a lower bound of the box lies above its upper bound");
        if (count == UVRT_MIRROR_MAX) return bad("a ninth panel (at most " + std::to_string(UVRT_MIRROR_MAX) + ")");
        uvrt_mirror& m = panelsOut[count++];
        memset(&m, 0, sizeof m);
        for (int k = 0; k < 3; ++k) { m.point[k] = q[k]; m.normal[k] = q[3 + k]; }
        m.reflectance = rho;
        for (size_t t = 0; t < T; ++t) {
            const float3_strict& c = tris[t].centroid;
            if (c.x >= v[0] && c.x <= v[3] && c.y >= v[1] && c.y <= v[4] && c.z >= v[2] && c.z <= v[5]) panelOfTriOut[t] = (uint8_t)count;
        }
    }
    *countOut = count;
    return std::string();
}

void RayTracer::SetMirrors(const uvrt_mirror* panels, int count, const uint8_t* panelOfTri, int triangleCount)
{
    if (count < 0 || count > UVRT_MIRROR_MAX || triangleCount < 0 || (count > 0 && (!panels || !panelOfTri)))
        fatal("SetMirrors: between 1 and 8 panels with a panel_of_tri, or nothing");
    mirrorPanels.assign(panels, panels + count);
    mirrorPanelOfTri.assign(panelOfTri, panelOfTri + (count > 0 ? triangleCount : 0));
    mirrorValuesStamp = mirrorStampNext++;
}

std::string RayTracer::MirrorMapPath() const
{
    return mirrorMap.empty() || mirrorMap[0] == '/' ? mirrorMap : routeDir + mirrorMap;
}

std::string RayTracer::PrepareMirrorMap()
{
    if (mirrorMap.empty()) return std::string();
    if (!mesh) return "mirrorMap: no mesh (Init comes first)";
    const std::string path = MirrorMapPath();
    if (mirrorFileParsed == path && mirrorFilePanelOfTri.size() == (size_t)mesh->triangleCount) return std::string();
    mirrorFileParsed.clear();
    mirrorFilePanels.assign(UVRT_MIRROR_MAX, uvrt_mirror{});
    mirrorFilePanelOfTri.assign((size_t)mesh->triangleCount, 0);
    int count = 0;
    const std::string err = ParseMirrorRules(path.c_str(), mesh->triangles, mesh->triangleCount, mirrorFilePanels.data(), &count,
                                             mirrorFilePanelOfTri.data());
    if (!err.empty()) { mirrorFilePanels.clear(); mirrorFilePanelOfTri.clear(); return err; }
    if (count == 0) { mirrorFilePanels.clear(); mirrorFilePanelOfTri.clear(); return path + ": no panel"; }
    mirrorFilePanels.resize((size_t)count);
    mirrorFileParsed = path;
    mirrorFileStamp = mirrorStampNext++;
    return std::string();
}

void RayTracer::UploadMirrors(int triangleCount)
{
    const std::string err = PrepareMirrorMap();
    if (!err.empty()) fatal(("mirrorMap: " + err).c_str());
    const bool file = !mirrorMap.empty();
    const std::vector<uvrt_mirror>& panels = file ? mirrorFilePanels : mirrorPanels;
    const std::vector<uint8_t>& members = file ? mirrorFilePanelOfTri : mirrorPanelOfTri;
    const unsigned long long stamp = file ? mirrorFileStamp : mirrorValuesStamp;
    if (panels.empty()) fatal("the mirror gather needs panels (mirrorMap or SetMirrors)");
    if (members.size() != (size_t)triangleCount) fatal("the panels' panel_of_tri must hold triangleCount entries");
    int32_t info[4];
    check(uvrt_mirror_info(ctx, info), "mirror_info");
    if (info[0] > 0 && mirrorUploaded == stamp) return;
    check(uvrt_set_mirrors(ctx, panels.data(), (int32_t)panels.size(), members.data()), "set_mirrors");
    mirrorUploaded = stamp;
}

// ------------------------------------------------------------ virtual dosimeters (raytracer.h sensorMap; raytracer_sensors.cpp)
const RayTracer::SensorHooks* RayTracer::sensorHooks = nullptr;

const RayTracer::SensorHooks& RayTracer::Sensors()
{
    if (!sensorHooks) fatal("sensors need host/raytracer_sensors.cpp in the program");
    return *sensorHooks;
}

void RayTracer::CheckSensorsAlone(const char* who) const
{
    auto refuse = [&](const char* why) { fatal((std::string(who) + ": " + why).c_str()); };
    if (shardWorld > 1) refuse("launch sharding (shardWorld > 1) is not supported with sensors");
    if (reduceOverComm) refuse("reduceOverComm is not supported with sensors (their maps live on one context)");
    if (HasMirrors()) refuse("mirror panels are not supported with sensors (a sensor would not see the panels' light)");
}

void RayTracer::ComputeSegments()
{
    std::vector<RouteLaunch> sweeps;
    for (const RouteLaunch& l : Launches())
        if (l.kind == UVRT_LAUNCH_SWEEP) sweeps.push_back(l);
    RunLaunches(sweeps, photonsPerLight, mesh->triangleCount, OwnGather(), false);
}

void RayTracer::RunLaunches(const std::vector<RouteLaunch>& list, int photons, int triangleCount, const GatherOptions& g, bool capture)
{
    if (const char* why = GatherRefusal(g, kBatchRefusals, false)) fatal(why);
    // (a refine that RunLaunch is about to refuse is left to it: its batch would be refused first, with another message)
    const bool refineOk = g.relError == 0.0 || (g.samples >= 2 && g.relError > 0.0 && std::isfinite(g.relError));
    if (g.batch < 2 || g.samples <= 0 || !refineOk) {
        for (const RouteLaunch& l : list) RunLaunch(l, photons, triangleCount, g, capture ? l.column : -1, -1);
        return;
    }
    // groups of up to g.batch consecutive launches: one shadow-ray pass each (include/uvrt.h uvrt_gather_direct_batch), then
    // every launch as RunLaunch runs it, with uvrt_gather_batch_select where uvrt_gather_direct stood
    const size_t batch = (size_t)g.batch;
    const long long want = std::min<long long>((long long)std::min(batch, list.size()) * triangleCount * g.samples, 1ll << 23);
    if (want > rayCapacity) {                                // results never depend on the capacity: the cap is a memory choice
        check(uvrt_resize_rays(ctx, want), "resize_rays");
        rayCapacity = want;
    }
    std::vector<uvrt_gather_params> params;
    for (size_t first = 0; first < list.size(); first += batch) {
        const size_t cnt = std::min(batch, list.size() - first);
        params.clear();
        for (size_t k = 0; k < cnt; ++k)                     // the seeds the launches take from gatherLaunches below
            params.push_back(gather_params(list[first + k], lightLength, g.samples, gatherLaunches + (unsigned)k, photons));
        check(uvrt_set_gather_sampling(ctx, g.sampling), "set_gather_sampling");
        {
            ScopedState variance(ctx, kVariancePlane, g.relError != 0.0);   // the refine reads the variance plane (RunLaunch)
            check(uvrt_gather_direct_batch(ctx, params.data(), (int32_t)cnt, 0, triangleCount), "gather_direct_batch");
        }
        for (size_t k = 0; k < cnt; ++k) {
            const RouteLaunch& l = list[first + k];
            RunLaunch(l, photons, triangleCount, g, capture ? l.column : -1, (int)k);
        }
    }
}

void RayTracer::RunLaunch(const RouteLaunch& l, int photons, int triangleCount, const GatherOptions& opt, int captureColumn, int batchSlot)
{
    const bool sweep = l.kind == UVRT_LAUNCH_SWEEP;
    if (const char* why = GatherRefusal(opt, kLaunchRefusals, false)) fatal(why);
    if (sweep && shardWorld > 1) fatal("driveSpeed > 0 is not supported with launch sharding (shardWorld > 1)");
    if (opt.sensors) CheckSensorsAlone("sensors");
    const int samples = opt.samples, sided = opt.sided, reflectS = opt.reflectSamples, reflectK = opt.reflectBounces;
    const float reflect = opt.reflectance;
    if (samples > 0) {
        // the direct gather: expected[t] for every triangle, then accumulate.cl on that plane (raytracer.h gatherSamples)
        if (shardWorld > 1) fatal("gatherSamples > 0 is not supported with launch sharding (shardWorld > 1)");
        const uvrt_gather_params g = gather_params(l, lightLength, samples, gatherLaunches++, photons);
        check(uvrt_set_gather_sampling(ctx, opt.sampling), "set_gather_sampling");
        {
            // the adaptive gather (raytracer.h gatherRelError): the variance plane on around the launch's planes, the refine after
            ScopedState variance(ctx, kVariancePlane, opt.relError != 0.0);
            // the launch's planes: taken from the batch that RunLaunches has traced (batchSlot >= 0), or traced here
            // (reflectSided: with the faces state on around it; the context's is put back)
            if (batchSlot >= 0) {
                check(uvrt_gather_batch_select(ctx, batchSlot), "gather_batch_select");
            } else {
                ScopedState faces(ctx, kFacePlanes, sided != 0);
                check(uvrt_gather_direct(ctx, &g, 0, triangleCount), "gather_direct");
            }
        }
        if (opt.relError != 0.0) {
            uvrt_refine_params rp;
            memset(&rp, 0, sizeof rp);
            rp.rel_error = opt.relError;
            rp.max_extra = opt.maxExtra;
            rp.seed = ~g.seed;
            check(uvrt_gather_refine(ctx, &rp, 0, triangleCount, nullptr), "gather_refine");
        }
        if (opt.mirrored) {
            // the specular panels (raytracer.h mirrorMap): the lamp's light by way of every panel, added to the finished direct
            // plane -- and, under reflectSided, to the face planes, so that the bounces below see it as a source
            UploadMirrors(triangleCount);
            ScopedState faces(ctx, kFacePlanes, sided != 0);
            check(uvrt_gather_mirror(ctx, &g, 1, 0, triangleCount), "gather_mirror");
        }
        if (reflect > 0.0f && reflectK > 0) {
            // reflectK bounces over recorded hit links (raytracer.h reflectBounces): traced once per scene and reflectS
            const uint32_t linkSeed = 0x85EBCA6Bu;
            int32_t info[4];
            check(uvrt_indirect_links_info(ctx, info), "indirect_links_info");
            if (info[0] != reflectS || (uint32_t)info[1] != linkSeed || info[3] != sided) {
                uvrt_links_params lp;
                memset(&lp, 0, sizeof lp);
                lp.samples = reflectS;
                lp.seed = linkSeed;
                if (sided) check(uvrt_indirect_links_build_sided(ctx, &lp), "indirect_links_build_sided");
                else check(uvrt_indirect_links_build(ctx, &lp), "indirect_links_build");
            }
            uvrt_linked_params kp;
            memset(&kp, 0, sizeof kp);
            kp.reflectance = reflect;
            kp.bounces = reflectK;
            kp.add = 1;
            if (opt.mapped) {
                // the face-resolved bounces with a reflectance per face (raytracer.h reflectMap): `reflect` is the map's base only
                UploadReflectanceMap(triangleCount, reflect);
                uvrt_mapped_params mp;
                memset(&mp, 0, sizeof mp);
                mp.bounces = reflectK;
                mp.add = 1;
                check(uvrt_gather_indirect_linked_mapped(ctx, &mp, 0, triangleCount), "gather_indirect_linked_mapped");
            } else if (sided) {
                // the face-resolved bounces (raytracer.h reflectSided): the gather's face planes are the emitter, no snapshot
                check(uvrt_gather_indirect_linked_sided(ctx, &kp, 0, triangleCount), "gather_indirect_linked_sided");
            } else {
                check(uvrt_indirect_source_from_expected(ctx), "indirect_source_from_expected");
                check(uvrt_gather_indirect_linked(ctx, &kp, 0, triangleCount), "gather_indirect_linked");
            }
        } else if (reflect > 0.0f) {
            // one diffuse bounce (raytracer.h reflectance): the finished direct plane is the emitter, its bounce is added to it
            uvrt_indirect_params ip;
            memset(&ip, 0, sizeof ip);
            ip.reflectance = reflect;
            ip.samples = reflectS;
            ip.seed = g.seed ^ 0x85EBCA6Bu;
            ip.add = 1;
            check(uvrt_indirect_source_from_expected(ctx), "indirect_source_from_expected");
            check(uvrt_gather_indirect(ctx, &ip, 0, triangleCount), "gather_indirect");
        }
        if (opt.sensors) (this->*Sensors().gather)(l, photons, opt, g.seed, true);
        if (captureColumn >= 0) check(uvrt_plan_capture_expected(ctx, captureColumn), "plan_capture_expected");
        check(uvrt_accumulate_expected(ctx, l.duration, triangleCount), "accumulate_expected");
    } else if (shardWorld <= 1 || (launchIndex % shardWorld) == shardRank) {
        if (sweep) check(uvrt_generate_sweep(ctx, l.from, l.to, lightLength, 0, photons), "generate_sweep");
        else check(uvrt_generate(ctx, l.from, lightLength, 0, photons), "generate");   // :78-80
        check(uvrt_extend(ctx, photons), "extend");                                    // :82
        if (opt.sensors) (this->*Sensors().gather)(l, photons, opt, 0u, true);
        check(uvrt_accumulate(ctx, l.duration, triangleCount), "accumulate");          // :84-85
    } else {
        // another rank traces this launch; keep generate.cl's program-scope SEED in step
        check(uvrt_advance_seed(ctx, l.from, lightLength), "advance_seed");
    }
    if (sweep) return;           // Shade divides by the photons per SOURCE (raytracer.h driveSpeed): a sweep adds none
    ++launchIndex;
    photonMapSize += photons;                                // :87
}

void RayTracer::ComputeSegmentDosageMap(LightPos a, LightPos b, int photonsPerLight, int triangleCount)
{
    if (!(driveSpeed > 0.0f)) fatal("ComputeSegmentDosageMap: driveSpeed must be > 0");
    RunLaunch(RouteLaunches({a, b}, mesh->floorHeight + lightHeight, driveSpeed).back(), photonsPerLight, triangleCount, OwnGather(), -1, -1);
}

void RayTracer::ComputeSingleLightDosageMap(LightPos lightPos, int photonsPerLight, int triangleCount)
{
    RunLaunch(RouteLaunches({lightPos}, mesh->floorHeight + lightHeight, 0.0f)[0], photonsPerLight, triangleCount, OwnGather(), -1, -1);
}

void RayTracer::SetRayRange(int rank, int world)
{
    // contiguous global-id ranges; the union over the ranks is [0, photonsPerLight)
    const long long n = photonsPerLight, share = (n + world - 1) / world;
    rangeFirst = std::min((long long)rank * share, n);
    rangeCount = std::min(share, n - rangeFirst);
}

void RayTracer::ComputeIterationsBatched(int iterations)
{
    std::vector<RayTracer*> self{this};
    ComputeIterationsBatched(self, iterations);
}

void RayTracer::ComputeIterationsBatched(const std::vector<RayTracer*>& group, int iterations)
{
    RayTracer* r0 = group[0];
    for (RayTracer* rt : group)
        if (rt->HasSensors() && !rt->planCapture)            // (a plan's capture runs no sensor call and leaves their maps alone)
            fatal("sensors are not supported by ComputeIterationsBatched (they are gathered launch by launch: ComputeDosageMap)");
    for (RayTracer* rt : group)
        if (rt->gatherSamples > 0) fatal("gatherSamples > 0 is not supported by ComputeIterationsBatched (the direct gather runs launch by launch: ComputeDosageMap)");
    bool driving = false;
    for (RayTracer* rt : group) driving = driving || rt->driveSpeed > 0.0f;
    if (driving) {
        // stops and segments go through uvrt_trace_batch_launches side by side; what stays per launch stays refused
        for (RayTracer* rt : group)
            if (!(rt->driveSpeed > 0.0f)) fatal("ComputeIterationsBatched: every instance of a group must drive (driveSpeed > 0) or none");
        if (r0->shardWorld > 1) fatal("driveSpeed > 0 is not supported with launch sharding (shardWorld > 1)");
    }
    TraceBatched(group, iterations);
}

// `iterations` x the route's launches in batches of up to 64; the last launch of an iteration carries its Shade
void RayTracer::TraceBatched(const std::vector<RayTracer*>& group, int iterations)
{
    std::vector<std::vector<RouteLaunch>> lists;             // built once per call; every instance's from its own fields
    for (RayTracer* rt : group) lists.push_back(rt->Launches());
    const int P = (int)lists[0].size();                      // launches per iteration
    const bool sweeps = P > 0 && lists[0].back().kind == UVRT_LAUNCH_SWEEP;
    const long long total = (long long)iterations * P;
    const int kMax = 64;                                  // launches per uvrt_trace_batch
    std::vector<float> lamps((size_t)kMax * 3);
    std::vector<uvrt_launch> launches((size_t)kMax);
    std::vector<std::vector<uvrt_replay_op>> ops(group.size(), std::vector<uvrt_replay_op>((size_t)kMax));
    std::vector<uvrt_ctx*> ctxs;
    for (RayTracer* rt : group) ctxs.push_back(rt->ctx);
    long long done = 0;
    while (done < total) {
        int cnt = (int)std::min<long long>(kMax, total - done);
        if (cnt < total - done && cnt >= P) cnt -= (int)((done + cnt) % P);    // end on an iteration where one fits
        for (size_t r = 0; r < group.size(); ++r) {
            RayTracer* rt = group[r];
            for (int j = 0; j < cnt; ++j) {
                const int pos = (int)((done + j) % P);
                const RouteLaunch& l = lists[r][pos];
                uvrt_launch& ln = launches[j];
                memset(&ln, 0, sizeof ln);
                memcpy(ln.from, l.from, 12);
                memcpy(ln.to, l.to, 12);
                ln.kind = l.kind;
                memcpy(&lamps[3 * j], l.from, 12);
                if (l.kind == UVRT_LAUNCH_STOP) {
                    rt->photonMapSize += rt->photonsPerLight;                     // :87
                    ++rt->launchIndex;
                }
                const ShadeArguments sh = rt->ShadeArgs();                       // (after the launch's photonMapSize +=)
                const bool shade = pos == P - 1;                                 // myapp.cpp:160
                ops[r][j] = {l.duration, shade, sh.which_map, sh.photons_per_light, sh.scaled_power, sh.min_value, rt->thresholdView};
                if (shade) {                                                     // myapp.cpp:162-163
                    ++rt->currIterations;
                    rt->progress = 100.0f * (float)rt->currIterations / (float)rt->maxIterations;
                }
            }
            const long long n = rt->rangeCount < 0 ? rt->photonsPerLight : rt->rangeCount;
            if (n <= 0) fatal("ComputeIterationsBatched: an empty ray range (more ranks than photons)");
            if (sweeps)
                check(uvrt_trace_batch_launches(rt->ctx, launches.data(), rt->lightLength, cnt, rt->rangeFirst, n), "trace_batch_launches");
            else
                check(uvrt_trace_batch(rt->ctx, lamps.data(), rt->lightLength, cnt, rt->rangeFirst, n), "trace_batch");
        }
        if (group.size() > 1) check(uvrt_reduce_batch_group(ctxs.data(), (int)ctxs.size()), "reduce_batch_group");
        for (size_t r = 0; r < group.size(); ++r) {
            RayTracer* rt = group[r];
            if (group.size() == 1 && rt->reduceOverComm) check(uvrt_reduce_batch(rt->ctx), "reduce_batch");
            if (rt->planCapture) {                       // launch j of the batch is column (done + j) % P
                std::vector<int32_t> pos((size_t)cnt);
                for (int j = 0; j < cnt; ++j) pos[j] = (int32_t)((done + j) % P);
                check(uvrt_plan_capture_batch(rt->ctx, pos.data(), cnt), "plan_capture_batch");
            }
            check(uvrt_replay_batch(rt->ctx, ops[r].data(), cnt, rt->mesh->triangleCount), "replay_batch");
        }
        done += cnt;
    }
}

uvrt_plan_report RayTracer::PlanDurations(const PlanOptions& opt, unsigned* seedOut)
{
    std::vector<RayTracer*> self{this};
    return PlanDurations(self, opt, seedOut);
}

// capture from photon counts: one batched computation on every instance of the group
void RayTracer::PlanCaptureCounts(const std::vector<RayTracer*>& group, int cols)
{
    for (RayTracer* rt : group) {
        check(uvrt_plan_begin(rt->ctx, cols), "plan_begin");
        rt->ClearBuffers(true);                              // ResetDosageMap without the route save
        rt->currIterations = 0;
        rt->launchIndex = 0;
        rt->planCapture = true;
    }
    ComputeIterationsBatched(group, group[0]->maxIterations);
    for (RayTracer* rt : group) rt->planCapture = false;
}

// capture from the direct gather: the launches of ComputeDosageMap with `g`, every plane into its column
// confidence z > 0: with the variance plane on and the exposure matrix's variance beside it, lowered to X - z sqrt(V) at the end
void RayTracer::PlanCaptureGather(const std::vector<RouteLaunch>& list, const GatherOptions& g, double confidence)
{
    if (shardWorld > 1 || reduceOverComm) fatal("PlanDurations: a plan from the direct gather does not shard (shardWorld > 1, reduceOverComm)");
    const bool bound = confidence > 0.0;
    ScopedState variance(ctx, kVariancePlane, bound);        // put back after the lowering, when the function ends
    if (bound) check(uvrt_plan_begin_expected_variance(ctx, (int)list.size()), "plan_begin_expected_variance");
    else check(uvrt_plan_begin_expected(ctx, (int)list.size()), "plan_begin_expected");
    ClearBuffers(true);                                      // ResetDosageMap without the route save
    currIterations = 0;
    launchIndex = 0;
    gatherLaunches = 0;
    for (int it = 0; it < maxIterations; ++it) {
        RunLaunches(list, photonsPerLight, mesh->triangleCount, g, true);
        Shade();
        ++currIterations;
    }
    if (bound) check(uvrt_plan_lower_confidence(ctx, confidence), "plan_lower_confidence");
}

// every instance solves on its own; the durations must agree, and a sweep's column must come back as it went in
std::vector<float> RayTracer::PlanSolve(const std::vector<RayTracer*>& group, const PlanOptions& opt, const std::vector<RouteLaunch>& list,
                                        uvrt_plan_report* rep, uvrt_plan_bounds_report* brep)
{
    RayTracer* r0 = group[0];
    const size_t cols = list.size(), L = r0->lightPositions.size();
    uvrt_plan_params prm;
    memset(&prm, 0, sizeof prm);
    prm.min_dose = opt.minDose >= 0.0f ? opt.minDose : r0->minDosage;
    prm.scaled_power = r0->lightIntensity * 0.1f;                 // raytracer.cpp:113
    prm.photons_per_position = (long long)r0->maxIterations * r0->photonsPerLight;   // photonMapSize / L at the end
    prm.min_photons = opt.minPhotons;
    prm.max_iterations = opt.maxIterations;
    prm.margin = opt.margin;
    prm.rel_gap = opt.relGap;
    prm.mask = opt.mask;
    // the bounds: a stop is free from 0, a sweep fixed at the duration its launch is accumulated with
    std::vector<float> lower(cols, 0.0f);
    std::vector<uint8_t> fixed(cols, 0);
    for (const RouteLaunch& l : list)
        if (l.kind == UVRT_LAUNCH_SWEEP) { lower[l.column] = l.duration; fixed[l.column] = 1; }
    uvrt_plan_bounds bounds;
    memset(&bounds, 0, sizeof bounds);
    bounds.lower = lower.data();
    bounds.fixed = fixed.data();
    memset(brep, 0, sizeof *brep);
    brep->free_columns = (int)L;
    std::vector<float> d(cols), d_other(cols);
    for (size_t r = 0; r < group.size(); ++r) {
        RayTracer* rt = group[r];
        uvrt_plan_report rr;
        float* dr = r == 0 ? d.data() : d_other.data();
        if (cols > L) check(uvrt_plan_solve_bounded(rt->ctx, &prm, &bounds, dr, &rr, r == 0 ? brep : nullptr), "plan_solve_bounded");
        else check(uvrt_plan_solve(rt->ctx, &prm, dr, &rr), "plan_solve");
        if (r == 0) *rep = rr;
        else if (memcmp(d.data(), d_other.data(), d.size() * 4) != 0) fatal("PlanDurations: the contexts of the group planned different durations");
    }
    if (memcmp(d.data() + L, lower.data() + L, (cols - L) * 4) != 0) fatal("PlanDurations: the solver changed the duration of a segment");
    return d;
}

uvrt_plan_report RayTracer::PlanDurations(const std::vector<RayTracer*>& group, const PlanOptions& opt, unsigned* seedOut)
{
    RayTracer* r0 = group[0];
    const int L = (int)r0->lightPositions.size();
    if (L == 0) fatal("PlanDurations: no positions");
    for (RayTracer* rt : group)
        if (rt->gatherSamples > 0) fatal("PlanDurations: gatherSamples > 0 is not supported (the exposure matrix holds photon counts)");
    // the columns of E are the route's launches: on a driving route the L - 1 segments follow the stops (raytracer.h)
    const std::vector<RouteLaunch> list = r0->Launches();
    if ((int)list.size() > L && L > 128) fatal("PlanDurations: a driving plan takes at most 128 positions (2L - 1 <= 256 columns)");
    if ((long long)r0->maxIterations * (long long)r0->photonsPerLight > 0xFFFFFFFFll)
        fatal("PlanDurations: iterations x photonsPerLight overflow the uint32 exposure counts");
    // what only a plan can get wrong, then what a plan shares with every launch (GatherRefusal)
    if (opt.gatherConfidence != 0.0) {
        if (!(opt.gatherConfidence > 0.0) || !std::isfinite(opt.gatherConfidence)) fatal("PlanDurations: gatherConfidence must be finite and >= 0");
        if (opt.gatherSamples < 2) fatal("PlanDurations: gatherConfidence needs a plan from the direct gather with gatherSamples >= 2");
        if (opt.mirrorMapped != 0)
            fatal("PlanDurations: mirrorMapped is not supported with gatherConfidence (the variance plane knows nothing of the specular part)");
        if (opt.reflectance != 0.0f)
            fatal("PlanDurations: reflectance is not supported with gatherConfidence (the variance plane knows nothing of the indirect part)");
    }
    if (opt.reflectMapped != 0 && opt.reflectMapped != 1) fatal("PlanDurations: reflectMapped must be 0 or 1");
    if (opt.mirrorMapped != 0 && opt.mirrorMapped != 1) fatal("PlanDurations: mirrorMapped must be 0 or 1");
    const GatherOptions gather = PlanGather(opt);
    if (const char* why = GatherRefusal(gather, kBatchRefusals | kLaunchRefusals, true)) fatal((std::string("PlanDurations: ") + why).c_str());
    if (opt.reflectMapped != 0 && !r0->HasReflectanceMap())
        fatal("PlanDurations: reflectMapped needs a reflectance map (RayTracer::reflectMap or SetReflectanceMap)");
    if (opt.mirrorMapped != 0 && !r0->HasMirrors()) fatal("PlanDurations: mirrorMapped needs specular panels (RayTracer::mirrorMap or SetMirrors)");
    uint32_t seed0 = 0;
    check(uvrt_get_seed(r0->ctx, &seed0), "get_seed");
    if (opt.gatherSamples > 0) {
        if (group.size() != 1) fatal("PlanDurations: a plan from the direct gather runs on one context (no group)");
        r0->PlanCaptureGather(list, gather, opt.gatherConfidence);
    } else {
        PlanCaptureCounts(group, (int)list.size());
    }
    uvrt_plan_report rep;
    uvrt_plan_bounds_report brep;
    const std::vector<float> d = PlanSolve(group, opt, list, &rep, &brep);
    for (RayTracer* rt : group) {
        for (int i = 0; i < L; ++i) rt->lightPositions[i].duration = d[i];
        rt->planBounds = brep;
        rt->planSegmentDurations.assign(d.begin() + L, d.end());
    }
    if (seedOut) *seedOut = seed0;
    return rep;
}

void RayTracer::EndPlan() { check(uvrt_plan_end(ctx), "plan_end"); }

void RayTracer::GridPositions(float xmin, float xmax, float zmin, float zmax, int nx, int nz, float inset, float* xz)
{
    const float x0 = xmin + inset, x1 = xmax - inset, z0 = zmin + inset, z1 = zmax - inset;
    for (int j = 0; j < nz; ++j)
        for (int i = 0; i < nx; ++i) {
            float* o = xz + 2 * ((size_t)j * nx + i);
            o[0] = nx == 1 ? 0.5f * (x0 + x1) : x0 + (x1 - x0) * (float)i / (float)(nx - 1);
            o[1] = nz == 1 ? 0.5f * (z0 + z1) : z0 + (z1 - z0) * (float)j / (float)(nz - 1);
        }
}

void RayTracer::SetCandidateGrid(int nx, int nz, float inset)
{
    if (nx < 1 || nz < 1) fatal("SetCandidateGrid: nx and nz must be >= 1");
    float xmin = INFINITY, xmax = -INFINITY, zmin = INFINITY, zmax = -INFINITY;
    for (int i = 0; i < mesh->triangleCount; ++i) {
        const Tri& t = mesh->triangles[i];
        for (const auto* v : {&t.vertex0, &t.vertex1, &t.vertex2}) {
            xmin = std::min(xmin, v->x); xmax = std::max(xmax, v->x);
            zmin = std::min(zmin, v->z); zmax = std::max(zmax, v->z);
        }
    }
    std::vector<float> xz((size_t)nx * nz * 2);
    GridPositions(xmin, xmax, zmin, zmax, nx, nz, inset, xz.data());
    lightPositions.clear();
    for (int k = 0; k < nx * nz; ++k) lightPositions.push_back({make_float2(xz[2 * k], xz[2 * k + 1]), 1.0f});
    UpdatePhotonsPerLight();
}

RayTracer::ShadeArguments RayTracer::ShadeArgs() const       // raytracer.cpp:96-116
{
    // only the photons of one iteration; x100: W/m^2 -> microW/cm^2
    if (viewMode == maxpower) return {UVRT_MAP_MAX, photonsPerLight, lightIntensity * 100, minPower};
    // x0.1: J/m^2 -> mJ/cm^2
    return {UVRT_MAP_SUM, photonMapSize / (int)lightPositions.size(), lightIntensity * 0.1f, minDosage};
}

void RayTracer::Shade()                                      // raytracer.cpp:93-120
{
    const ShadeArguments a = ShadeArgs();
    check(uvrt_shade(ctx, a.which_map, a.photons_per_light, a.scaled_power, a.min_value, thresholdView, mesh->triangleCount),
          "computeDosage + dosageToColor");
}

void RayTracer::ResetDosageMap()                             // raytracer.cpp:122-131
{
    startedComputation = true;
    compTime = 0;
    timerClock.reset();
    if (autoSaveRoute) SaveRoute(defaultRouteFile);
    progress = 0;
    finishedComputation = false;
    currIterations = 0;
    launchIndex = 0;
    gatherLaunches = 0;
    ClearBuffers(true);
    if (HasSensors()) (this->*Sensors().reset)();             // the sensors' maps and their launch counter with the triangles'
}

void RayTracer::ClearBuffers(bool resetColor)                // raytracer.cpp:133-143
{
    photonMapSize = 0;
    check(uvrt_resize_rays(ctx, photonCount), "resize_rays");
    rayCapacity = photonCount;
    check(uvrt_reset(ctx, resetColor), "reset");
}

void RayTracer::CalibratePower(float measurePower, float measureHeight, float measureDist)   // :151-227
{
    measureHeight += mesh->floorHeight;

    // A small square as the sample geometry, 0.2 m wide, facing the lamp
    LightPos singleLightPos;
    singleLightPos.position = make_float2(0.0f, 0.0f);
    singleLightPos.duration = 0.0f;   // uninitialised in the reference; only the max map is read
    Tri square[2];
    memset((void*)square, 0, sizeof square);
    const float triWidth = 0.1f;
    const float x = singleLightPos.position.x, z = singleLightPos.position.y + measureDist;
    square[0].vertex0 = make_float3_strict(x + triWidth, measureHeight + triWidth, z);
    square[0].vertex1 = make_float3_strict(x - triWidth, measureHeight + triWidth, z);
    square[0].vertex2 = make_float3_strict(x + triWidth, measureHeight - triWidth, z);
    square[1].vertex0 = make_float3_strict(x - triWidth, measureHeight - triWidth, z);
    square[1].vertex1 = make_float3_strict(x - triWidth, measureHeight + triWidth, z);
    square[1].vertex2 = make_float3_strict(x + triWidth, measureHeight - triWidth, z);
    // single-node BVH whose root is a leaf (raytracer.cpp:173-187); its bounds are never tested
    BVHNode hostNode;
    memset(&hostNode, 0, sizeof hostNode);
    hostNode.leftFirst = 0;
    hostNode.triCount = 2;
    uint hostTriIdx[2] = {0, 1};
    check(uvrt_set_scene(ctx, square, 2, &hostNode, 1, hostTriIdx), "set_scene(calibration)");

    const int keepRank = shardRank, keepWorld = shardWorld;
    const long long keepIndex = launchIndex;
    shardRank = 0;
    shardWorld = 1;   // calibration is replicated: every rank traces every launch
    ClearBuffers(false);
    for (int i = 0; i < maxIterations; ++i)
        ComputeSingleLightDosageMap(singleLightPos, photonCount, 2);
    shardRank = keepRank;
    shardWorld = keepWorld;
    launchIndex = keepIndex;

    // power 1, so measured / traced irradiance is the calibrated power
    check(uvrt_compute_dosage(ctx, UVRT_MAP_MAX, photonCount, 1.0f, 2), "computeDosage");
    check(uvrt_sync(ctx), "sync");
    check(uvrt_read_dosage(ctx, dosageMap, 0, 2), "read_dosage");
    const float avgPower = (dosageMap[0] + dosageMap[1]) / 2.0f;
    calibratedPower = 0.01f * (measurePower / avgPower);
    lightIntensity = calibratedPower;

    // restore the room (raytracer.cpp:212-224)
    check(uvrt_set_scene(ctx, mesh->triangles, mesh->triangleCount, mesh->bvh->bvhNode,
                         (int)mesh->bvh->nodesUsed, mesh->bvh->triIdx), "set_scene(restore)");
    std::cout << "Done calibrating " << std::endl;
}

void RayTracer::ReadDosage(float* out, int first, int count)
{
    check(uvrt_read_dosage(ctx, out, first, count), "read_dosage");
}

void RayTracer::Sync() { check(uvrt_sync(ctx), "sync"); }

void RayTracer::SaveRoute(char fileName[32])                 // raytracer.cpp:233-259
{
    // Same document tinyxml2 prints: 4-space indent, floats as "%.8g".
    std::ostringstream o;
    o << "<route>\n";
    o << "    <aantal_fotonen>" << photonCount << "</aantal_fotonen>\n";
    o << "    <aantal_iteraties>" << maxIterations << "</aantal_iteraties>\n";
    o << "    <lamp_sterkte>" << float_str(lightIntensity) << "</lamp_sterkte>\n";
    o << "    <minimale_dosis>" << float_str(minDosage) << "</minimale_dosis>\n";
    o << "    <minimale_bestralingssterkte>" << float_str(minPower) << "</minimale_bestralingssterkte>\n";
    if (driveSpeed > 0.0f) o << "    <rijsnelheid>" << float_str(driveSpeed) << "</rijsnelheid>\n";   // (not in the reference's files)
    if (gatherSamples > 0) o << "    <gather_samples>" << gatherSamples << "</gather_samples>\n";                  // (likewise)
    if (gatherSamples > 0 && gatherSampling > 0) o << "    <gather_sampling>" << gatherSampling << "</gather_sampling>\n";
    if (reflectance > 0.0f) {
        o << "    <reflectance>" << float_str(reflectance) << "</reflectance>\n";
        o << "    <reflect_samples>" << reflectSamples << "</reflect_samples>\n";
        if (reflectBounces > 0) o << "    <reflect_bounces>" << reflectBounces << "</reflect_bounces>\n";
        if (reflectBounces > 0 && reflectSided != 0) o << "    <reflect_sided>1</reflect_sided>\n";
        if (reflectBounces > 0 && reflectSided != 0 && !reflectMap.empty()) {
            if (reflectMap.find_first_of("<>&") != std::string::npos) fatal("reflectMap: a file name with <, > or & cannot stand in a route file");
            o << "    <reflect_map>" << reflectMap << "</reflect_map>\n";
        }
    }
    if (!mirrorMap.empty()) {                                // the last gather tag
        if (mirrorMap.find_first_of("<>&") != std::string::npos) fatal("mirrorMap: a file name with <, > or & cannot stand in a route file");
        o << "    <mirror_map>" << mirrorMap << "</mirror_map>\n";
    }
    if (!sensorMap.empty()) {                                // (no gather tag: photon launches gather sensors too)
        if (sensorMap.find_first_of("<>&") != std::string::npos) fatal("sensorMap: a file name with <, > or & cannot stand in a route file");
        o << "    <sensor_map>" << sensorMap << "</sensor_map>\n";
        o << "    <sensor_samples>" << sensorSamples << "</sensor_samples>\n";
    }
    o << "    <lamp_lengte>" << float_str(lightLength) << "</lamp_lengte>\n";
    o << "    <lamp_hoogte>" << float_str(lightHeight) << "</lamp_hoogte>\n";
    if (lightPositions.empty()) o << "    <route/>\n";
    else {
        o << "    <route>\n";
        for (size_t i = 0; i < lightPositions.size(); i++) {
            const LightPos& lp = lightPositions[i];
            o << "        <lamp_positie_" << i << " positie_x=\"" << float_str(lp.position.x) << "\" positie_y=\""
              << float_str(lp.position.y) << "\" duration=\"" << float_str(lp.duration) << "\"/>\n";
        }
        o << "    </route>\n";
    }
    o << "</route>\n";
    std::ofstream f(routeDir + fileName + ".xml", std::ios::binary);
    if (f) f << o.str();   // a failed save is silent in the reference too (return value dropped)
}

void RayTracer::LoadRoute(char fileName[32])                 // raytracer.cpp:261-300
{
    std::ifstream f(routeDir + fileName + ".xml", std::ios::binary);
    if (!f) return;                                          // :266
    std::stringstream ss;
    ss << f.rdbuf();
    const std::string text = ss.str();
    XmlParser xp(text);
    XmlElem root;
    if (!xp.element(root)) return;
    const XmlElem* e;
    if ((e = root.child("aantal_fotonen"))) to_int(trim(e->text), &photonCount);
    if ((e = root.child("aantal_iteraties"))) to_int(trim(e->text), &maxIterations);
    if ((e = root.child("lamp_sterkte"))) to_float(trim(e->text), &lightIntensity);
    if ((e = root.child("minimale_dosis"))) to_float(trim(e->text), &minDosage);
    if ((e = root.child("minimale_bestralingssterkte"))) to_float(trim(e->text), &minPower);
    driveSpeed = 0.0f;
    if ((e = root.child("rijsnelheid"))) to_float(trim(e->text), &driveSpeed);
    gatherSamples = 0;
    if ((e = root.child("gather_samples"))) to_int(trim(e->text), &gatherSamples);
    gatherSampling = 0;
    if ((e = root.child("gather_sampling"))) to_int(trim(e->text), &gatherSampling);
    reflectance = 0.0f;
    if ((e = root.child("reflectance"))) to_float(trim(e->text), &reflectance);
    reflectSamples = 16;
    if ((e = root.child("reflect_samples"))) to_int(trim(e->text), &reflectSamples);
    reflectBounces = 0;
    if ((e = root.child("reflect_bounces"))) to_int(trim(e->text), &reflectBounces);
    reflectSided = 0;
    if ((e = root.child("reflect_sided"))) to_int(trim(e->text), &reflectSided);
    reflectMap.clear();                                      // (the file's cache goes with the name it belongs to)
    reflectFileValues.clear();
    reflectFileParsed.clear();
    if ((e = root.child("reflect_map"))) reflectMap = trim(e->text);
    mirrorMap.clear();                                       // (likewise)
    mirrorFilePanels.clear();
    mirrorFilePanelOfTri.clear();
    mirrorFileParsed.clear();
    if ((e = root.child("mirror_map"))) mirrorMap = trim(e->text);
    sensorMap.clear();                                       // (likewise)
    sensorFileList.clear();
    sensorFileParsed.clear();
    if ((e = root.child("sensor_map"))) sensorMap = trim(e->text);
    sensorSamples = 64;
    if ((e = root.child("sensor_samples"))) to_int(trim(e->text), &sensorSamples);
    if ((e = root.child("lamp_lengte"))) to_float(trim(e->text), &lightLength);
    if ((e = root.child("lamp_hoogte"))) to_float(trim(e->text), &lightHeight);
    if ((e = root.child("route"))) {
        lightPositions.clear();
        for (int i = 0;; i++) {
            const XmlElem* lampElem = e->child("lamp_positie_" + std::to_string(i));
            if (!lampElem) break;
            LightPos lp;
            lp.position = make_float2(0.0f, 0.0f);
            lp.duration = 0.0f;
            const std::string* a;
            if ((a = lampElem->attr("positie_x"))) to_float(*a, &lp.position.x);
            if ((a = lampElem->attr("positie_y"))) to_float(*a, &lp.position.y);
            if ((a = lampElem->attr("duration"))) to_float(*a, &lp.duration);
            lightPositions.push_back(lp);
        }
    }
    UpdatePhotonsPerLight();
}

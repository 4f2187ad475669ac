// host_calls_check.cpp -- the host layer's call sequence, without a GPU (tests/test_host_calls_cpu.py).
//
// host/raytracer.cpp decides which uvrt_* call runs with which seed.  This program links it (with host/mesh.cpp and
// host/bvh.cpp) against recording stand-ins for every uvrt_* function it calls: a stand-in appends one line -- its name, the
// context's number, then every scalar argument and every field of a params struct in the order include/uvrt.h declares them,
// floats as hex bit patterns, arrays as their byte length and an FNV-1a hash -- and returns UVRT_OK.  The stand-ins keep the little state the host's decisions read: the
// variance and faces flags, what the links / reflectance / mirror info calls report, a seed, and a plan solve that writes
// d[i] = i + 1 into free columns and the lower bound into fixed ones.
//
// Every case drives the public RayTracer API over a 12-triangle box with three positions and prints what was recorded; the
// refusals run in a forked child whose stderr line and exit status are recorded.  Without an argument all cases are printed,
// with a case's name that one alone.  tests/golden/host_call_sequences.txt is the whole output.
#include "raytracer.h"

#include <omp.h>
#include <sys/wait.h>
#include <unistd.h>

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <string>
#include <vector>

using namespace Tmpl8;

// ------------------------------------------------------------ the recording stand-ins
struct uvrt_ctx {
    int id = 0, variance = 0, faces = 0, reflectance = 0, mirrors = 0, columns = 0, triangles = 0;
    int32_t links[4] = {0, 0, 0, 0};                          // samples, seed, built, sided
};

namespace {

std::string record;
int contexts = 0;
FILE* out = nullptr;                                         // the record goes here (main)

void put(const char* fmt, ...)
{
    char line[1024];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(line, sizeof line, fmt, ap);
    va_end(ap);
    record += line;
    record += '\n';
}
unsigned F(float v) { unsigned u; memcpy(&u, &v, 4); return u; }
unsigned long long D(double v) { unsigned long long u; memcpy(&u, &v, 8); return u; }
std::string A(const void* p, size_t bytes)                   // an array: its length in bytes and FNV-1a over them
{
    if (!p) return "null";
    unsigned h = 2166136261u;
    for (size_t i = 0; i < bytes; ++i) h = (h ^ ((const unsigned char*)p)[i]) * 16777619u;
    char b[48];
    snprintf(b, sizeof b, "%zu:%08x", bytes, h);
    return b;
}
std::string V3(const float* v)
{
    char b[48];
    snprintf(b, sizeof b, "%08x,%08x,%08x", F(v[0]), F(v[1]), F(v[2]));
    return b;
}
std::string G(const uvrt_gather_params& g)
{
    char b[256];
    snprintf(b, sizeof b, "%s %s %08x %d %08x %d %d,%d", V3(g.from).c_str(), V3(g.to).c_str(),
             F(g.light_length), g.samples, g.seed, g.photons_equiv, g.reserved[0], g.reserved[1]);
    return b;
}
std::string plan_params(const uvrt_ctx* c, const uvrt_plan_params* p)
{
    char b[320];
    snprintf(b, sizeof b, "%08x %08x %lld %d %d %016llx %016llx %s "
             "%d,%d", F(p->min_dose), F(p->scaled_power), (long long)p->photons_per_position, p->min_photons, p->max_iterations,
             D(p->margin), D(p->rel_gap), A(p->mask, (size_t)c->triangles).c_str(), p->reserved[0], p->reserved[1]);
    return b;
}
void solve(uvrt_ctx* c, const uvrt_plan_bounds* bounds, float* d, uvrt_plan_report* rep)
{
    for (int i = 0; i < c->columns; ++i) d[i] = bounds && bounds->fixed[i] ? bounds->lower[i] : (float)(i + 1);
    memset(rep, 0, sizeof *rep);
    rep->positions = c->columns;
}

}  // namespace

extern "C" {

const char* uvrt_last_error(void) { return "(stand-in)"; }
int uvrt_create(int device_id, uvrt_ctx** out)
{
    *out = new uvrt_ctx();
    (*out)->id = contexts++;
    put("create c%d %d", (*out)->id, device_id);
    return UVRT_OK;
}
void uvrt_destroy(uvrt_ctx* c) { put("destroy c%d", c->id); delete c; }
int uvrt_set_scene(uvrt_ctx* c, const void* tris64, int32_t tri_count, const void* nodes32, int32_t node_count, const uint32_t* tri_idx)
{
    put("set_scene c%d %d/%s %d/%s %s", c->id, tri_count, A(tris64, (size_t)tri_count * 64).c_str(), node_count,
        A(nodes32, (size_t)node_count * 32).c_str(), A(tri_idx, (size_t)tri_count * 4).c_str());
    c->triangles = tri_count;
    c->reflectance = c->mirrors = 0;                         // a scene swap drops the links, the map and the panels
    memset(c->links, 0, sizeof c->links);
    return UVRT_OK;
}
int uvrt_resize_rays(uvrt_ctx* c, int64_t n) { put("resize_rays c%d %lld", c->id, (long long)n); return UVRT_OK; }
int uvrt_reset(uvrt_ctx* c, int32_t color) { put("reset c%d %d", c->id, color); return UVRT_OK; }
int uvrt_sync(uvrt_ctx* c) { put("sync c%d", c->id); return UVRT_OK; }
int uvrt_get_seed(uvrt_ctx* c, uint32_t* seed) { *seed = 0x5EED0000u + (unsigned)c->id; put("get_seed c%d", c->id); return UVRT_OK; }
int uvrt_read_dosage(uvrt_ctx* c, float* out, int32_t first, int32_t count)
{
    put("read_dosage c%d %d %d", c->id, first, count);
    for (int i = 0; i < count; ++i) out[i] = 1.0f;
    return UVRT_OK;
}

// photons
int uvrt_generate(uvrt_ctx* c, const float pos[3], float len, int64_t first, int64_t n)
{
    put("generate c%d %s %08x %lld %lld", c->id, V3(pos).c_str(), F(len), (long long)first, (long long)n);
    return UVRT_OK;
}
int uvrt_generate_sweep(uvrt_ctx* c, const float from[3], const float to[3], float len, int64_t first, int64_t n)
{
    put("generate_sweep c%d %s %s %08x %lld %lld", c->id, V3(from).c_str(), V3(to).c_str(), F(len), (long long)first,
        (long long)n);
    return UVRT_OK;
}
int uvrt_advance_seed(uvrt_ctx* c, const float pos[3], float len) { put("advance_seed c%d %s %08x", c->id, V3(pos).c_str(), F(len)); return UVRT_OK; }
int uvrt_extend(uvrt_ctx* c, int64_t n) { put("extend c%d %lld", c->id, (long long)n); return UVRT_OK; }
int uvrt_accumulate(uvrt_ctx* c, float dt, int32_t tris) { put("accumulate c%d %08x %d", c->id, F(dt), tris); return UVRT_OK; }
int uvrt_accumulate_expected(uvrt_ctx* c, float dt, int32_t tris) { put("accumulate_expected c%d %08x %d", c->id, F(dt), tris); return UVRT_OK; }
int uvrt_compute_dosage(uvrt_ctx* c, int32_t map, int32_t ppl, float power, int32_t tris)
{
    put("compute_dosage c%d %d %d %08x %d", c->id, map, ppl, F(power), tris);
    return UVRT_OK;
}
int uvrt_shade(uvrt_ctx* c, int32_t map, int32_t ppl, float power, float min_value, int32_t threshold, int32_t tris)
{
    put("shade c%d %d %d %08x %08x %d %d", c->id, map, ppl, F(power), F(min_value), threshold, tris);
    return UVRT_OK;
}

// batched tracing
int uvrt_trace_batch(uvrt_ctx* c, const float* lamps, float len, int32_t count, int64_t first, int64_t n)
{
    put("trace_batch c%d %s %08x %d %lld %lld", c->id, A(lamps, (size_t)count * 12).c_str(), F(len), count,
        (long long)first, (long long)n);
    return UVRT_OK;
}
int uvrt_trace_batch_launches(uvrt_ctx* c, const uvrt_launch* l, float len, int32_t count, int64_t first, int64_t n)
{
    put("trace_batch_launches c%d %s %08x %d %lld %lld", c->id, A(l, (size_t)count * sizeof *l).c_str(), F(len),
        count, (long long)first, (long long)n);
    return UVRT_OK;
}
int uvrt_reduce_batch(uvrt_ctx* c) { put("reduce_batch c%d", c->id); return UVRT_OK; }
int uvrt_reduce_batch_group(uvrt_ctx** cs, int32_t n)
{
    std::string ids;
    for (int i = 0; i < n; ++i) ids += " c" + std::to_string(cs[i]->id);
    put("reduce_batch_group%s", ids.c_str());
    return UVRT_OK;
}
int uvrt_replay_batch(uvrt_ctx* c, const uvrt_replay_op* ops, int32_t count, int32_t tris)
{
    put("replay_batch c%d %s %d %d", c->id, A(ops, (size_t)count * sizeof *ops).c_str(), count, tris);
    return UVRT_OK;
}

// the gathers
int uvrt_set_gather_sampling(uvrt_ctx* c, int32_t mode) { put("set_gather_sampling c%d %d", c->id, mode); return UVRT_OK; }
int uvrt_get_gather_variance(uvrt_ctx* c, int32_t* on) { *on = c->variance; put("get_gather_variance c%d -> %d", c->id, *on); return UVRT_OK; }
int uvrt_set_gather_variance(uvrt_ctx* c, int32_t on) { c->variance = on; put("set_gather_variance c%d %d", c->id, on); return UVRT_OK; }
int uvrt_get_gather_faces(uvrt_ctx* c, int32_t* on) { *on = c->faces; put("get_gather_faces c%d -> %d", c->id, *on); return UVRT_OK; }
int uvrt_set_gather_faces(uvrt_ctx* c, int32_t on) { c->faces = on; put("set_gather_faces c%d %d", c->id, on); return UVRT_OK; }
int uvrt_gather_direct(uvrt_ctx* c, const uvrt_gather_params* g, int32_t first, int32_t tris)
{
    put("gather_direct c%d %s %d %d", c->id, G(*g).c_str(), first, tris);
    return UVRT_OK;
}
int uvrt_gather_direct_batch(uvrt_ctx* c, const uvrt_gather_params* g, int32_t count, int32_t first, int32_t tris)
{
    put("gather_direct_batch c%d %d %d %d", c->id, count, first, tris);
    for (int k = 0; k < count; ++k) put("  launch %d %s", k, G(g[k]).c_str());
    return UVRT_OK;
}
int uvrt_gather_batch_select(uvrt_ctx* c, int32_t k) { put("gather_batch_select c%d %d", c->id, k); return UVRT_OK; }
int uvrt_gather_refine(uvrt_ctx* c, const uvrt_refine_params* p, int32_t first, int32_t tris, uvrt_refine_report* report)
{
    put("gather_refine c%d %016llx %016llx %d %08x %d,%d %d %d %d", c->id,
        D(p->rel_error), D(p->min_expected), p->max_extra, p->seed, p->reserved[0], p->reserved[1], first, tris, report != nullptr);
    return UVRT_OK;
}
int uvrt_gather_mirror(uvrt_ctx* c, const uvrt_gather_params* g, int32_t add, int32_t first, int32_t tris)
{
    put("gather_mirror c%d %s %d %d %d", c->id, G(*g).c_str(), add, first, tris);
    return UVRT_OK;
}
int uvrt_mirror_info(uvrt_ctx* c, int32_t out4[4])
{
    out4[0] = c->mirrors; out4[1] = out4[2] = out4[3] = 0;
    put("mirror_info c%d -> %d", c->id, out4[0]);
    return UVRT_OK;
}
int uvrt_set_mirrors(uvrt_ctx* c, const uvrt_mirror* panels, int32_t count, const uint8_t* panel_of_tri)
{
    put("set_mirrors c%d %s %d %s", c->id, A(panels, (size_t)count * sizeof *panels).c_str(), count,
        A(panel_of_tri, (size_t)c->triangles).c_str());
    c->mirrors = count;
    return UVRT_OK;
}
int uvrt_indirect_source_from_expected(uvrt_ctx* c) { put("indirect_source_from_expected c%d", c->id); return UVRT_OK; }
int uvrt_gather_indirect(uvrt_ctx* c, const uvrt_indirect_params* p, int32_t first, int32_t tris)
{
    put("gather_indirect c%d %08x %d %08x %d %d,%d %d %d", c->id, F(p->reflectance), p->samples,
        p->seed, p->add, p->reserved[0], p->reserved[1], first, tris);
    return UVRT_OK;
}
int uvrt_indirect_links_info(uvrt_ctx* c, int32_t out4[4])
{
    memcpy(out4, c->links, sizeof c->links);
    put("indirect_links_info c%d -> %d %08x %d %d", c->id, out4[0], (unsigned)out4[1], out4[2], out4[3]);
    return UVRT_OK;
}
static int links_build(uvrt_ctx* c, const uvrt_links_params* p, int sided)
{
    put("indirect_links_build%s c%d %d %08x %d,%d", sided ? "_sided" : "", c->id, p->samples, p->seed, p->reserved[0],
        p->reserved[1]);
    c->links[0] = p->samples; c->links[1] = (int32_t)p->seed; c->links[2] = 1; c->links[3] = sided;
    return UVRT_OK;
}
int uvrt_indirect_links_build(uvrt_ctx* c, const uvrt_links_params* p) { return links_build(c, p, 0); }
int uvrt_indirect_links_build_sided(uvrt_ctx* c, const uvrt_links_params* p) { return links_build(c, p, 1); }
static int linked(const char* name, uvrt_ctx* c, const uvrt_linked_params* p, int32_t first, int32_t tris)
{
    put("%s c%d %08x %d %d %d,%d,%d %d %d", name, c->id, F(p->reflectance), p->bounces, p->add,
        p->reserved[0], p->reserved[1], p->reserved[2], first, tris);
    return UVRT_OK;
}
int uvrt_gather_indirect_linked(uvrt_ctx* c, const uvrt_linked_params* p, int32_t first, int32_t tris)
{ return linked("gather_indirect_linked", c, p, first, tris); }
int uvrt_gather_indirect_linked_sided(uvrt_ctx* c, const uvrt_linked_params* p, int32_t first, int32_t tris)
{ return linked("gather_indirect_linked_sided", c, p, first, tris); }
int uvrt_gather_indirect_linked_mapped(uvrt_ctx* c, const uvrt_mapped_params* p, int32_t first, int32_t tris)
{
    put("gather_indirect_linked_mapped c%d %d %d %d,%d %d %d", c->id, p->bounces, p->add, p->reserved[0],
        p->reserved[1], first, tris);
    return UVRT_OK;
}
int uvrt_reflectance_info(uvrt_ctx* c, int32_t* have) { *have = c->reflectance; put("reflectance_info c%d -> %d", c->id, *have); return UVRT_OK; }
int uvrt_write_reflectance(uvrt_ctx* c, int32_t face, const float* in, int32_t first, int32_t count)
{
    put("write_reflectance c%d %d %s %d %d", c->id, face, A(in, (size_t)count * 4).c_str(), first, count);
    c->reflectance = 1;
    return UVRT_OK;
}

// planning
static int begin(const char* name, uvrt_ctx* c, int32_t positions) { c->columns = positions; put("%s c%d %d", name, c->id, positions); return UVRT_OK; }
int uvrt_plan_begin(uvrt_ctx* c, int32_t positions) { return begin("plan_begin", c, positions); }
int uvrt_plan_begin_expected(uvrt_ctx* c, int32_t positions) { return begin("plan_begin_expected", c, positions); }
int uvrt_plan_begin_expected_variance(uvrt_ctx* c, int32_t positions) { return begin("plan_begin_expected_variance", c, positions); }
int uvrt_plan_capture_batch(uvrt_ctx* c, const int32_t* pos, int32_t count)
{
    put("plan_capture_batch c%d %s %d", c->id, A(pos, (size_t)count * 4).c_str(), count);
    return UVRT_OK;
}
int uvrt_plan_capture_expected(uvrt_ctx* c, int32_t position) { put("plan_capture_expected c%d %d", c->id, position); return UVRT_OK; }
int uvrt_plan_lower_confidence(uvrt_ctx* c, double z) { put("plan_lower_confidence c%d %016llx", c->id, D(z)); return UVRT_OK; }
int uvrt_plan_end(uvrt_ctx* c) { put("plan_end c%d", c->id); return UVRT_OK; }
int uvrt_plan_solve(uvrt_ctx* c, const uvrt_plan_params* p, float* d, uvrt_plan_report* rep)
{
    put("plan_solve c%d %s", c->id, plan_params(c, p).c_str());
    solve(c, nullptr, d, rep);
    return UVRT_OK;
}
int uvrt_plan_solve_bounded(uvrt_ctx* c, const uvrt_plan_params* p, const uvrt_plan_bounds* b, float* d, uvrt_plan_report* rep,
                            uvrt_plan_bounds_report* brep)
{
    put("plan_solve_bounded c%d %s %s %s %d,%d %d", c->id, plan_params(c, p).c_str(),
        A(b->lower, (size_t)c->columns * 4).c_str(), A(b->fixed, (size_t)c->columns).c_str(), b->reserved[0], b->reserved[1], brep != nullptr);
    solve(c, b, d, rep);
    if (brep) {
        memset(brep, 0, sizeof *brep);
        for (int i = 0; i < c->columns; ++i) (b->fixed[i] ? brep->fixed_columns : brep->free_columns)++;
    }
    return UVRT_OK;
}

}  // extern "C"

// ------------------------------------------------------------ the scene and the cases
namespace {

// a box of 12 triangles, x and z in [-2, 2], y in [0, 3]
std::vector<Tri> box()
{
    const float c[8][3] = {{-2, 0, -2}, {2, 0, -2}, {2, 0, 2}, {-2, 0, 2}, {-2, 3, -2}, {2, 3, -2}, {2, 3, 2}, {-2, 3, 2}};
    const int quads[6][4] = {{0, 1, 2, 3}, {4, 5, 6, 7}, {0, 1, 5, 4}, {1, 2, 6, 5}, {2, 3, 7, 6}, {3, 0, 4, 7}};
    std::vector<Tri> tris(12);
    memset((void*)tris.data(), 0, sizeof(Tri) * tris.size());
    for (int q = 0; q < 6; ++q)
        for (int h = 0; h < 2; ++h) {
            const int* k = quads[q];
            const int v[3] = {k[0], k[h ? 2 : 1], k[h ? 3 : 2]};
            Tri& t = tris[2 * q + h];
            t.vertex0 = make_float3_strict(c[v[0]][0], c[v[0]][1], c[v[0]][2]);
            t.vertex1 = make_float3_strict(c[v[1]][0], c[v[1]][1], c[v[1]][2]);
            t.vertex2 = make_float3_strict(c[v[2]][0], c[v[2]][1], c[v[2]][2]);
        }
    return tris;
}

// one ray tracer over the box: three positions, 64 photons per light, two iterations, no route file
struct Scene {
    Mesh mesh;
    RayTracer rt;
    Scene()
    {
        const std::vector<Tri> tris = box();
        mesh.SetTriangles(tris.data(), (int)tris.size());
        rt.routeDir = "/nonexistent/";
        rt.autoSaveRoute = false;
        rt.Init(&mesh);
        rt.lightPositions = {{make_float2(-1.0f, -1.0f), 1.5f}, {make_float2(0.0f, 0.5f), 2.0f}, {make_float2(1.0f, 1.0f), 0.5f}};
        rt.photonCount = 192;
        rt.UpdatePhotonsPerLight();
        rt.maxIterations = 2;
    }
    void map() { const std::vector<float> rho(24, 0.25f); rt.SetReflectanceMap(rho.data(), 24); }
    void mirrors()
    {
        uvrt_mirror m;
        memset(&m, 0, sizeof m);
        m.point[0] = 2.0f; m.normal[0] = -1.0f; m.reflectance = 0.75f;
        const std::vector<uint8_t> of(12, 0);
        rt.SetMirrors(&m, 1, of.data(), 12);
    }
    // what MyApp::Tick does for one iteration
    void iterate() { rt.ComputeDosageMap(); rt.Shade(); ++rt.currIterations; }
    void reset_and_iterate() { rt.ResetDosageMap(); iterate(); }
};

typedef std::function<void(Scene&)> Body;
struct Case { std::string name; Body body; bool refusal; };
std::vector<Case> cases;
void run(const std::string& name, Body body) { cases.push_back({name, body, false}); }
void refuse(const std::string& name, Body body) { cases.push_back({name, body, true}); }

// RayTracer members for a gather with S samples
void gather(Scene& s, int S) { s.rt.gatherSamples = S; }
void bounce(Scene& s, float rho, int K, int sided) { s.rt.reflectance = rho; s.rt.reflectBounces = K; s.rt.reflectSided = sided; }

RayTracer::PlanOptions gather_plan(int S)
{
    RayTracer::PlanOptions o;
    o.minDose = 50.0f;
    o.gatherSamples = S;
    return o;
}
void plan(Scene& s, const RayTracer::PlanOptions& o)
{
    unsigned seed = 0;
    const uvrt_plan_report rep = s.rt.PlanDurations(o, &seed);
    put("-> seed=%08x positions=%d durations=%08x,%08x,%08x segments=%zu", seed, rep.positions, F(s.rt.lightPositions[0].duration),
        F(s.rt.lightPositions[1].duration), F(s.rt.lightPositions[2].duration), s.rt.planSegmentDurations.size());
}

void list_cases()
{
    // ---- ComputeDosageMap and its kin
    // every way a launch gathers, as a stop (one iteration of the three positions) and while driving (the two segments)
    const std::pair<const char*, Body> ways[] = {
        {"photons", [](Scene&) {}},
        {"gather", [](Scene& s) { gather(s, 4); }},
        {"gather stratified", [](Scene& s) { gather(s, 4); s.rt.gatherSampling = 1; }},
        {"gather refine", [](Scene& s) { gather(s, 4); s.rt.gatherRelError = 0.125; s.rt.gatherMaxExtra = 32; }},
        {"gather traced bounce", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 0, 0); s.rt.reflectSamples = 8; }},
        {"gather sided bounces", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 1); }},
        {"gather sided mapped bounces", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 1); s.map(); }},
        {"gather mirrors", [](Scene& s) { gather(s, 4); s.mirrors(); }},
        {"gather mirrors sided", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 1); s.mirrors(); }},
        {"gather batch 2", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 2; }},
        {"gather batch 64", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 64; }},
        {"gather batch 2 refine", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 2; s.rt.gatherRelError = 0.125; }},
        {"gather batch 2 mirrors", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 2; s.mirrors(); }},
        {"gather batch 64 refine mirrors linked", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 64; s.rt.gatherRelError = 0.125; s.mirrors();
                                                                 bounce(s, 0.5f, 3, 0); }},
    };
    for (const auto& w : ways) {
        const Body set = w.second;
        run(std::string("stops: ") + w.first, [set](Scene& s) { set(s); s.reset_and_iterate(); });
        run(std::string("segments: ") + w.first, [set](Scene& s) { set(s); s.rt.driveSpeed = 0.5f; s.rt.ResetDosageMap(); s.rt.ComputeSegments(); });
    }
    run("photons driving, two iterations", [](Scene& s) { s.rt.driveSpeed = 0.5f; s.reset_and_iterate(); s.iterate(); });
    for (int rank = 0; rank < 2; ++rank)
        run("photons sharded, rank " + std::to_string(rank), [rank](Scene& s) { s.rt.shardRank = rank; s.rt.shardWorld = 2; s.reset_and_iterate(); s.iterate(); });
    run("gather linked bounces, two iterations", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 0); s.reset_and_iterate(); s.iterate(); });
    run("gather linked then sided then another sample count", [](Scene& s) {
        gather(s, 4); bounce(s, 0.5f, 2, 0); s.reset_and_iterate();
        s.rt.reflectSided = 1; s.iterate();
        s.rt.reflectSamples = 32; s.iterate();
    });
    run("gather mapped: a second map, then a scene swap", [](Scene& s) {
        gather(s, 4); bounce(s, 0.5f, 2, 1); s.map(); s.mirrors(); s.reset_and_iterate();
        s.map(); s.iterate();
        s.rt.Init(&s.mesh); s.rt.ResetDosageMap(); s.iterate();
    });
    run("gather driving, everything", [](Scene& s) {
        gather(s, 4); s.rt.gatherSampling = 1; s.rt.gatherRelError = 0.125; bounce(s, 0.5f, 2, 1); s.map(); s.mirrors(); s.rt.driveSpeed = 0.5f;
        s.reset_and_iterate();
    });
    run("variance and faces on before the launch", [](Scene& s) {
        uvrt_set_gather_variance(s.rt.ctx, 1); uvrt_set_gather_faces(s.rt.ctx, 1);
        gather(s, 4); s.rt.gatherRelError = 0.125; bounce(s, 0.5f, 2, 1); s.mirrors(); s.reset_and_iterate();
    });
    run("single launches", [](Scene& s) {
        gather(s, 4); s.rt.gatherRelError = 0.125; s.rt.gatherBatch = 65; s.rt.driveSpeed = 0.5f;      // (a single launch reads no batch)
        s.rt.ResetDosageMap();
        s.rt.ComputeSingleLightDosageMap(s.rt.lightPositions[1], 32, 12);
        s.rt.ComputeSegmentDosageMap(s.rt.lightPositions[0], s.rt.lightPositions[2], 32, 12);
        s.rt.gatherSamples = 0; s.rt.gatherRelError = 0.0;
        s.rt.ComputeSingleLightDosageMap(s.rt.lightPositions[1], 32, 12);
        s.rt.ComputeSegmentDosageMap(s.rt.lightPositions[0], s.rt.lightPositions[2], 32, 12);
    });
    run("no launch, nothing refused but the batch", [](Scene& s) {               // ComputeSegments at driveSpeed 0: an empty list
        s.rt.reflectBounces = 17; s.rt.gatherRelError = -1.0; s.rt.reflectance = 2.0f; s.mirrors(); s.rt.ResetDosageMap(); s.rt.ComputeSegments();
    });

    // ---- PlanDurations
    run("plan: counts", [](Scene& s) { RayTracer::PlanOptions o; o.minPhotons = 8; o.margin = 1e-5; o.relGap = 1e-2; o.maxIterations = 50; plan(s, o); });
    run("plan: counts with a mask, the route's minimum", [](Scene& s) {
        const std::vector<unsigned char> mask = {1, 1, 0, 0, 1, 1, 1, 1, 0, 1, 1, 1};
        RayTracer::PlanOptions o; o.mask = mask.data(); plan(s, o);
    });
    run("plan: counts, driving", [](Scene& s) { s.rt.driveSpeed = 0.5f; RayTracer::PlanOptions o; o.minDose = 50.0f; plan(s, o); s.rt.EndPlan(); });
    run("plan: counts, a group of two", [](Scene& s) {
        Scene other;
        s.rt.SetRayRange(0, 2); other.rt.SetRayRange(1, 2);
        RayTracer::PlanOptions o; o.minDose = 50.0f;
        unsigned seed = 0;
        const uvrt_plan_report rep = RayTracer::PlanDurations({&s.rt, &other.rt}, o, &seed);
        put("-> seed=%08x positions=%d durations=%08x,%08x", seed, rep.positions, F(s.rt.lightPositions[0].duration), F(other.rt.lightPositions[2].duration));
    });
    run("plan: counts over a communicator", [](Scene& s) { s.rt.reduceOverComm = true; RayTracer::PlanOptions o; plan(s, o); });
    run("plan: gather", [](Scene& s) { plan(s, gather_plan(4)); });
    run("plan: gather stratified, driving", [](Scene& s) { s.rt.driveSpeed = 0.5f; RayTracer::PlanOptions o = gather_plan(4); o.gatherSampling = 1; plan(s, o); });
    run("plan: gatherConfidence", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherConfidence = 2.0; plan(s, o); });
    run("plan: gatherConfidence, variance on before", [](Scene& s) {
        uvrt_set_gather_variance(s.rt.ctx, 1); RayTracer::PlanOptions o = gather_plan(4); o.gatherConfidence = 2.0; o.gatherRelError = 0.25; plan(s, o);
    });
    run("plan: gatherRelError", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherRelError = 0.25; o.gatherMaxExtra = 16; plan(s, o); });
    run("plan: reflectance", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.reflectSamples = 8; plan(s, o); });
    run("plan: reflectBounces", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.reflectBounces = 2; plan(s, o); });
    run("plan: reflectSided", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.reflectBounces = 2; o.reflectSided = 1; plan(s, o); });
    run("plan: reflectMapped", [](Scene& s) {
        s.map(); RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.reflectBounces = 2; o.reflectSided = 1; o.reflectMapped = 1; plan(s, o);
    });
    run("plan: a map and panels the plan does not ask for", [](Scene& s) { s.map(); s.mirrors(); plan(s, gather_plan(4)); });
    run("plan: mirrorMapped", [](Scene& s) { s.mirrors(); RayTracer::PlanOptions o = gather_plan(4); o.mirrorMapped = 1; plan(s, o); });
    run("plan: gatherBatch", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherBatch = 2; plan(s, o); });
    run("plan: the ray tracer's own gather knobs are not the plan's", [](Scene& s) {
        s.rt.gatherSampling = 1; s.rt.gatherRelError = 0.5; bounce(s, 0.5f, 2, 1); s.rt.gatherBatch = 2; plan(s, gather_plan(4));
    });
    run("plan: everything together", [](Scene& s) {
        s.map(); s.mirrors(); s.rt.driveSpeed = 0.5f;
        RayTracer::PlanOptions o = gather_plan(4);
        o.gatherSampling = 1; o.gatherRelError = 0.25; o.reflectance = 0.5f; o.reflectSamples = 8; o.reflectBounces = 2; o.reflectSided = 1;
        o.reflectMapped = 1; o.mirrorMapped = 1; o.gatherBatch = 1;
        plan(s, o);
    });
    run("plan: everything a batch takes together", [](Scene& s) {
        s.mirrors();
        RayTracer::PlanOptions o = gather_plan(4);
        o.gatherSampling = 1; o.gatherRelError = 0.25; o.reflectance = 0.5f; o.reflectBounces = 2; o.mirrorMapped = 1; o.gatherBatch = 64;
        plan(s, o);
    });

    // ---- refusals of a launch: one state per condition, each otherwise sound
    refuse("launch: reflectBounces range", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 17, 0); s.reset_and_iterate(); });
    refuse("launch: reflectBounces negative", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, -1, 0); s.reset_and_iterate(); });
    refuse("launch: gatherBatch range", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 65; s.reset_and_iterate(); });
    refuse("launch: gatherBatch range, no launch", [](Scene& s) { s.rt.gatherBatch = -1; s.rt.ResetDosageMap(); s.rt.ComputeSegments(); });
    refuse("launch: reflectSided value", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 2); s.reset_and_iterate(); });
    refuse("launch: reflectSided needs reflectance", [](Scene& s) { gather(s, 4); bounce(s, 0.0f, 2, 1); s.reset_and_iterate(); });
    refuse("launch: reflectSided needs reflectBounces", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 0, 1); s.reset_and_iterate(); });
    refuse("launch: reflectSided with gatherBatch", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 1); s.rt.gatherBatch = 2; s.reset_and_iterate(); });
    refuse("launch: reflectSided with gatherBatch, no launch", [](Scene& s) {
        gather(s, 4); bounce(s, 0.5f, 2, 1); s.rt.gatherBatch = 2; s.rt.ResetDosageMap(); s.rt.ComputeSegments();
    });
    refuse("launch: reflectMap needs reflectSided", [](Scene& s) { gather(s, 4); bounce(s, 0.5f, 2, 0); s.map(); s.reset_and_iterate(); });
    refuse("launch: a sweep with sharding", [](Scene& s) { s.rt.driveSpeed = 0.5f; s.rt.shardWorld = 2; s.rt.ResetDosageMap(); s.rt.ComputeSegments(); });
    refuse("launch: a gather with sharding", [](Scene& s) { gather(s, 4); s.rt.shardWorld = 2; s.reset_and_iterate(); });
    refuse("launch: gatherRelError needs gatherSamples", [](Scene& s) { gather(s, 1); s.rt.gatherRelError = 0.125; s.reset_and_iterate(); });
    refuse("launch: gatherRelError with photons", [](Scene& s) { s.rt.gatherRelError = 0.125; s.reset_and_iterate(); });
    refuse("launch: gatherRelError negative", [](Scene& s) { gather(s, 4); s.rt.gatherRelError = -0.125; s.reset_and_iterate(); });
    refuse("launch: gatherRelError not finite", [](Scene& s) { gather(s, 4); s.rt.gatherRelError = INFINITY; s.reset_and_iterate(); });
    refuse("launch: gatherRelError negative, in a batch", [](Scene& s) { gather(s, 4); s.rt.gatherBatch = 2; s.rt.gatherRelError = -0.125; s.reset_and_iterate(); });
    refuse("launch: reflectance needs gatherSamples", [](Scene& s) { bounce(s, 0.5f, 0, 0); s.reset_and_iterate(); });
    refuse("launch: reflectance above 1", [](Scene& s) { gather(s, 4); bounce(s, 1.5f, 0, 0); s.reset_and_iterate(); });
    refuse("launch: reflectance negative", [](Scene& s) { gather(s, 4); bounce(s, -0.5f, 0, 0); s.reset_and_iterate(); });
    refuse("launch: reflectance not a number", [](Scene& s) { gather(s, 4); bounce(s, NAN, 0, 0); s.reset_and_iterate(); });
    refuse("launch: mirrorMap needs gatherSamples", [](Scene& s) { s.mirrors(); s.reset_and_iterate(); });
    refuse("launch: a segment without driveSpeed", [](Scene& s) { s.rt.ComputeSegmentDosageMap(s.rt.lightPositions[0], s.rt.lightPositions[1], 32, 12); });

    // ---- refusals of a plan
    auto sided_plan = [] { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.reflectBounces = 2; o.reflectSided = 1; return o; };
    refuse("plan: no positions", [](Scene& s) { s.rt.lightPositions.clear(); plan(s, gather_plan(4)); });
    refuse("plan: the ray tracer's gatherSamples", [](Scene& s) { gather(s, 4); plan(s, gather_plan(4)); });
    refuse("plan: driving with more than 128 positions", [](Scene& s) {
        s.rt.lightPositions.assign(129, s.rt.lightPositions[0]); s.rt.driveSpeed = 0.5f; plan(s, gather_plan(4));
    });
    refuse("plan: exposure counts overflow", [](Scene& s) { s.rt.photonsPerLight = 1 << 20; s.rt.maxIterations = 5000; plan(s, gather_plan(4)); });
    refuse("plan: gatherConfidence negative", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherConfidence = -1.0; plan(s, o); });
    refuse("plan: gatherConfidence not finite", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherConfidence = INFINITY; plan(s, o); });
    refuse("plan: gatherConfidence needs gatherSamples", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(1); o.gatherConfidence = 2.0; plan(s, o); });
    refuse("plan: gatherRelError negative", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherRelError = -0.25; plan(s, o); });
    refuse("plan: gatherRelError not finite", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherRelError = NAN; plan(s, o); });
    refuse("plan: gatherRelError needs gatherSamples", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(1); o.gatherRelError = 0.25; plan(s, o); });
    refuse("plan: reflectBounces range", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.reflectBounces = 17; plan(s, o); });
    refuse("plan: reflectBounces negative", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectBounces = -1; plan(s, o); });
    refuse("plan: gatherBatch range", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.gatherBatch = 65; plan(s, o); });
    refuse("plan: gatherBatch negative", [](Scene& s) { RayTracer::PlanOptions o; o.gatherBatch = -1; plan(s, o); });
    refuse("plan: reflectSided value", [sided_plan](Scene& s) { RayTracer::PlanOptions o = sided_plan(); o.reflectSided = 2; plan(s, o); });
    refuse("plan: reflectSided needs reflectance", [sided_plan](Scene& s) { RayTracer::PlanOptions o = sided_plan(); o.reflectance = 0.0f; plan(s, o); });
    refuse("plan: reflectSided needs reflectBounces", [sided_plan](Scene& s) { RayTracer::PlanOptions o = sided_plan(); o.reflectBounces = 0; plan(s, o); });
    refuse("plan: reflectSided with gatherBatch", [sided_plan](Scene& s) { RayTracer::PlanOptions o = sided_plan(); o.gatherBatch = 2; plan(s, o); });
    refuse("plan: reflectMapped value", [sided_plan](Scene& s) { s.map(); RayTracer::PlanOptions o = sided_plan(); o.reflectMapped = 2; plan(s, o); });
    refuse("plan: reflectMapped needs reflectSided", [sided_plan](Scene& s) {
        s.map(); RayTracer::PlanOptions o = sided_plan(); o.reflectSided = 0; o.reflectMapped = 1; plan(s, o);
    });
    refuse("plan: reflectMapped needs a map", [sided_plan](Scene& s) { RayTracer::PlanOptions o = sided_plan(); o.reflectMapped = 1; plan(s, o); });
    refuse("plan: mirrorMapped value", [](Scene& s) { s.mirrors(); RayTracer::PlanOptions o = gather_plan(4); o.mirrorMapped = 2; plan(s, o); });
    refuse("plan: mirrorMapped needs gatherSamples", [](Scene& s) { s.mirrors(); RayTracer::PlanOptions o = gather_plan(0); o.mirrorMapped = 1; plan(s, o); });
    refuse("plan: mirrorMapped with gatherConfidence", [](Scene& s) {
        s.mirrors(); RayTracer::PlanOptions o = gather_plan(4); o.mirrorMapped = 1; o.gatherConfidence = 2.0; plan(s, o);
    });
    refuse("plan: mirrorMapped needs panels", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.mirrorMapped = 1; plan(s, o); });
    refuse("plan: reflectance above 1", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 1.5f; plan(s, o); });
    refuse("plan: reflectance negative", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(4); o.reflectance = -0.5f; plan(s, o); });
    refuse("plan: reflectance needs gatherSamples", [](Scene& s) { RayTracer::PlanOptions o = gather_plan(0); o.reflectance = 0.5f; plan(s, o); });
    refuse("plan: reflectance with gatherConfidence", [](Scene& s) {
        RayTracer::PlanOptions o = gather_plan(4); o.reflectance = 0.5f; o.gatherConfidence = 2.0; plan(s, o);
    });
    refuse("plan: a gather plan on a group", [](Scene& s) { Scene other; RayTracer::PlanDurations({&s.rt, &other.rt}, gather_plan(4), nullptr); });
    refuse("plan: a gather plan with sharding", [](Scene& s) { s.rt.shardWorld = 2; plan(s, gather_plan(4)); });
    refuse("plan: a gather plan over a communicator", [](Scene& s) { s.rt.reduceOverComm = true; plan(s, gather_plan(4)); });
}

// a case's record: what the stand-ins saw between the scene's set-up and its end
std::string recorded(const Case& c)
{
    contexts = 0;
    {
        Scene s;
        record.clear();                                      // (the set-up is the same for every case: "set-up" records it once)
        c.body(s);
    }
    return record;
}

// a refusal: the call in a child, its stderr and how it ended
std::string refused(const Case& c)
{
    int fds[2];
    if (pipe(fds) != 0) return "pipe failed\n";
    fflush(out);                                             // (or the child would print what is buffered once more)
    const pid_t pid = fork();
    if (pid < 0) return "fork failed\n";
    if (pid == 0) {
        close(fds[0]);
        dup2(fds[1], 2);
        Scene s;
        c.body(s);
        _exit(0);                                            // nothing refused it
    }
    close(fds[1]);
    std::string err;
    char buf[512];
    for (ssize_t n; (n = read(fds[0], buf, sizeof buf)) > 0;) err.append(buf, (size_t)n);
    close(fds[0]);
    int status = 0;
    waitpid(pid, &status, 0);
    char head[64];
    if (WIFEXITED(status)) snprintf(head, sizeof head, "exit %d: ", WEXITSTATUS(status));
    else snprintf(head, sizeof head, "signal %d: ", WTERMSIG(status));
    return head + err + (err.empty() || err.back() != '\n' ? "\n" : "");
}

}  // namespace

int main(int argc, char** argv)
{
    omp_set_num_threads(1);                                  // the BVH build without a thread pool: a forked child can build one too
    out = fdopen(dup(1), "w");                               // the record alone: what Mesh prints about itself is not part of it
    if (!out || !freopen("/dev/null", "w", stdout)) return 3;
    list_cases();
    cases.insert(cases.begin(), {"set-up", [](Scene&) {}, false});
    bool found = false;
    for (const Case& c : cases) {
        if (argc > 1 && c.name != argv[1]) continue;
        found = true;
        std::string text;
        if (c.name == "set-up") {                            // Init and the scene, once; every other case starts after it
            contexts = 0;
            record.clear();
            { Scene s; }
            text = record;
        } else {
            text = c.refusal ? refused(c) : recorded(c);
        }
        fprintf(out, "== %s\n%s", c.name.c_str(), text.c_str());
    }
    if (!found) { fprintf(stderr, "no case '%s'\n", argv[1]); return 2; }
    return fclose(out) == 0 ? 0 : 3;
}

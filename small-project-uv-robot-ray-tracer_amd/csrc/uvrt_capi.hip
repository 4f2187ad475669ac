// uvrt_capi.hip -- context, scene, buffers, knobs, read-backs and test hooks
// (the C ABI of include/uvrt.h over the HIP kernels; the context and its helpers are in uvrt_ctx.h)
#include "uvrt_ctx.h"
#include "uvrt_scene_layout.h"

#include <climits>
#include <cstddef>

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

thread_local std::string g_err;

int fail(int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    g_err = buf;
    return code;
}

}  // namespace uvrt_impl

// (the streams are idle: uvrt_destroy has waited for them; a failed uvrt_create has enqueued zero fills only, which hipFree waits for)
uvrt_ctx::~uvrt_ctx()
{
    plan_drop(this);
    (void)hot_reset(this, false);
    for (hipEvent_t e : {ev_fence, ev_mapfence}) if (e) (void)hipEventDestroy(e);
    for (hipEvent_t e : ev_pool) (void)hipEventDestroy(e);
    if (host_flag) (void)hipHostFree(host_flag);
    if (probe_stream) (void)hipStreamDestroy(probe_stream);
    if (own_stream) (void)hipStreamDestroy(own_stream);
}

namespace {

namespace sl = uvrt::scene_layout;
using sl::SceneLayout;

// the layout's records are uploaded as the device's, byte for byte, and its constants are the device's
#define SAME_FIELD(A, B, f) (offsetof(A, f) == offsetof(B, f))
static_assert(sizeof(sl::F4) == sizeof(float4) && SAME_FIELD(sl::F4, float4, x) && SAME_FIELD(sl::F4, float4, y) &&
              SAME_FIELD(sl::F4, float4, z) && SAME_FIELD(sl::F4, float4, w), "F4 is float4's words");
static_assert(sizeof(sl::PairWords) == sizeof(PairRec) && SAME_FIELD(sl::PairWords, PairRec, c0min_ref0) &&
              SAME_FIELD(sl::PairWords, PairRec, c0max_ref1) && SAME_FIELD(sl::PairWords, PairRec, c1min) &&
              SAME_FIELD(sl::PairWords, PairRec, c1max), "PairWords is PairRec");
static_assert(sizeof(sl::QuadWords) == sizeof(QuadRec) && SAME_FIELD(sl::QuadWords, QuadRec, xz) && SAME_FIELD(sl::QuadWords, QuadRec, y01) &&
              SAME_FIELD(sl::QuadWords, QuadRec, y23) && SAME_FIELD(sl::QuadWords, QuadRec, ref) && SAME_FIELD(sl::QuadWords, QuadRec, pad),
              "QuadWords is QuadRec");
#undef SAME_FIELD
static_assert(sl::REF_LEAF_BIT == uvrt::REF_LEAF_BIT && sl::REF_DONE == uvrt::REF_DONE && sl::REF_COUNT_SHIFT == uvrt::REF_COUNT_SHIFT &&
              sl::MAX_TRIS == uvrt::MAX_TRIS && sl::TOP6_MAX == uvrt::TOP6_MAX, "uvrt_scene_layout.h restates uvrt_device.h's constants");

// An environment knob: the integer in `name`, where it is set and lies in [lo, hi], into `field`; true when it was taken.
template <class I>
bool env_int(const char* name, long lo, long hi, I& field)
{
    const char* e = getenv(name);
    if (!e) return false;
    const long v = atol(e);
    if (v < lo || v > hi) return false;
    field = (I)v;
    return true;
}
// ... and an on / off knob: anything but 0 is on
void env_bool(const char* name, bool& field)
{
    if (const char* e = getenv(name)) field = atoi(e) != 0;
}

// the scene's buffers and, where T changes, the per-triangle maps (the streams are joined and idle)
int provision_scene(uvrt_ctx* c, const SceneLayout& L, int32_t T)
{
    const bool resized = (T != c->T);
    int rc;
    if ((rc = c->pairs.ensure(std::max<size_t>(L.pairs.size(), 1) * sizeof(PairRec), false, c->stream))) return rc;
    for (int l = 0; l < c->nlanes; ++l)
        if ((rc = c->lanes[l].recs.ensure((L.pairs.size() + (size_t)T + 1) * 64, true, c->stream))) return rc;
    // + 16 bytes: the merged record fetch of the traversal reads 64 bytes at every leaf record
    if ((rc = c->ltris.ensure((size_t)T * sizeof(LeafTri) + 16, true, c->stream))) return rc;
    if ((rc = c->leaf_count.ensure((size_t)T * 4, false, c->stream))) return rc;
    if ((rc = c->area.ensure((size_t)T * 4, false, c->stream))) return rc;
    if (resized || !c->photon_map.p) {
        // raytracer.cpp:32-37 (the reference leaves them uninitialised until reset; zero here)
        // The colour buffer stands for the GL vertex buffer of the caller's mesh (raytracer.cpp:37): a scene swap
        // does not touch it.  It only grows, so CalibratePower's detour over a 2-triangle scene
        // (raytracer.cpp:166-224, ClearBuffers(false)) leaves the room's colours as they were.
        for (DevBuf* b : {&c->photon_map, &c->max_map, &c->dosage}) b->release();
        for (Lane& La : c->lanes) La.counts.release();
        if ((rc = c->photon_map.ensure((size_t)T * 8, true, c->stream))) return rc;
        if ((rc = c->max_map.ensure((size_t)T * 8, true, c->stream))) return rc;
        // 16 deposit replicas (two per XCD: a workgroup deposits into replica blockIdx % 16), at most 64 MiB in
        // total.  Fewer than 8 serialise on the hot triangles' counters; more than ~24 push the planes out of L2 and
        // every wave then waits for its deposits' memory round trips (profiles/r02/r02_experiments.txt: 64 replicas cost
        // the batched step 5 %)
        int R = c->replicas_knob > 0 ? c->replicas_knob : 16;
        while (R > 1 && (size_t)R * (size_t)T * 4 > ((size_t)64 << 20)) R >>= 1;
        c->replicas = R;
        for (int l = 0; l < c->nlanes; ++l)
            if ((rc = c->lanes[l].counts.ensure((size_t)R * (size_t)T * 4, true, c->stream))) return rc;
        if ((rc = c->dosage.ensure((size_t)T * 4, true, c->stream))) return rc;
        if ((rc = c->color.ensure((size_t)T * 36, true, c->stream))) return rc;
    }
    return UVRT_OK;
}

// the layout and the caller's arrays to the device, the two preparation kernels, and the scene's scalars once they have run
int upload_scene(uvrt_ctx* c, const SceneLayout& L, const void* tris64, int32_t T, const uint32_t* tri_idx)
{
    int rc;
    if (!L.pairs.empty())
        HIP_TRY(hipMemcpyAsync(c->pairs.p, L.pairs.data(), L.pairs.size() * sizeof(PairRec), hipMemcpyHostToDevice, c->stream));
    if ((rc = c->quads.ensure(std::max<size_t>(L.quads.size(), 1) * sizeof(QuadRec), false, c->stream))) return rc;
    if (!L.quads.empty())
        HIP_TRY(hipMemcpyAsync(c->quads.p, L.quads.data(), L.quads.size() * sizeof(QuadRec), hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->leaf_count.p, L.leaf_count.data(), (size_t)T * 4, hipMemcpyHostToDevice, c->stream));
    // staging copies of the reference-layout arrays for the device-side preparation kernel
    DevBuf d_tris, d_idx;
    if ((rc = d_tris.ensure((size_t)T * 64, false, c->stream))) return rc;
    if ((rc = d_idx.ensure((size_t)T * 4, false, c->stream))) return rc;
    HIP_TRY(hipMemcpyAsync(d_tris.p, tris64, (size_t)T * 64, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(d_idx.p, tri_idx, (size_t)T * 4, hipMemcpyHostToDevice, c->stream));
    launch_prepare_scene(d_tris.as<float4>(), d_idx.as<uint32_t>(), c->ltris.as<LeafTri>(),
                         c->area.as<float>(), T, c->stream);
    for (int l = 0; l < c->nlanes; ++l)
        launch_prepare_leaves6(c->ltris.as<LeafTri>(), c->lanes[l].recs.p, (int32_t)L.pairs.size(), T, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->T = T;
    c->root_ref = L.root_ref;
    c->top_pairs = L.top_pairs;
    c->npairs = (int32_t)L.pairs.size();
    c->nquads = (int32_t)L.quads.size();
    c->top_quads = L.top_quads;
    c->scene_force_exact = L.force_exact;
    c->have_scene = true;
    return UVRT_OK;
}

// Whatever an earlier scene left in the context is void.  What is made on first use goes whole (uvrt_ctx::SceneDerived:
// nothing to list); each of the rest has a reason to be handled on its own.
int void_scene_state(uvrt_ctx* c)
{
    for (Lane& La : c->lanes) { La.recs_tag.valid = false; La.recs4_tag.valid = false; }   // the buffers stay, their contents are stale
    for (Lane& La : c->lanes) La.recs4.release();     // sized per scene; rebuilt on demand (uvrt_set_wide_bvh)
    c->have_perm = false;                             // the caller's renumbering: `perm` is reused by the next one
    c->derived = {};
    if (int rc = hot_reset(c, true)) return rc;       // statistics of the previous scene; the new scene's first slab
    HIP_TRY(hipStreamSynchronize(c->stream));
    plan_drop(c);                                     // E is per scene
    // a batch of the previous scene is void; its buffers are sized per scene
    c->b_count = 0;
    c->b_is_folded = false;
    c->b_recs.clear();
    c->b_recs_key.clear();
    for (auto& bset : c->bs) for (DevBuf* b : {&bset.planes, &bset.folded}) b->release();
    return UVRT_OK;
}

}  // namespace

extern "C" {

const char* uvrt_last_error(void) { return g_err.c_str(); }
const char* uvrt_version(void) { return "uvrt-mi355x 0.1 (gfx950)"; }
int uvrt_clock_probe_start(uvrt_ctx* c, int32_t microseconds)
{
    if (!c || microseconds < 1 || microseconds > 1000000) return fail(UVRT_ERR_INVALID, "uvrt_clock_probe_start: 1 .. 1 000 000 us");
    HIP_TRY(hipSetDevice(c->device));
    if (!c->probe_stream) {
        int lo = 0, hi = 0;
        HIP_TRY(hipDeviceGetStreamPriorityRange(&lo, &hi));
        HIP_TRY(hipStreamCreateWithPriority(&c->probe_stream, hipStreamNonBlocking, hi));     // a wave slot as soon as one frees
    }
    if (int rc = c->probe_out.ensure(16, true, c->probe_stream)) return rc;
    launch_clock_probe(c->probe_out.as<unsigned long long>(), (unsigned long long)microseconds * 100ull, c->probe_stream);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

int uvrt_clock_probe_read(uvrt_ctx* c, double* shader_mhz)
{
    if (!c || !shader_mhz || !c->probe_stream) return fail(UVRT_ERR_INVALID, "uvrt_clock_probe_read: no probe started");
    HIP_TRY(hipSetDevice(c->device));
    unsigned long long v[2] = {0, 0};
    HIP_TRY(hipMemcpyAsync(v, c->probe_out.p, 16, hipMemcpyDeviceToHost, c->probe_stream));
    HIP_TRY(hipStreamSynchronize(c->probe_stream));
    if (v[1] == 0) return fail(UVRT_ERR_HIP, "uvrt_clock_probe_read: the probe wrote nothing");
    *shader_mhz = (double)v[0] / (double)v[1] * 100.0;          // s_memrealtime ticks at 100 MHz
    return UVRT_OK;
}

int uvrt_device_cus(uvrt_ctx* c) { return c ? c->num_cus : 0; }
int uvrt_device_count(void)
{
    int n = 0;
    return hipGetDeviceCount(&n) == hipSuccess ? n : 0;
}

int uvrt_create(int device_id, uvrt_ctx** out)
{
    if (!out) return fail(UVRT_ERR_INVALID, "uvrt_create: out is NULL");
    *out = nullptr;
    int ndev = 0;
    hipError_t e = hipGetDeviceCount(&ndev);
    if (e != hipSuccess || ndev <= 0)
        return fail(UVRT_ERR_NO_DEVICE, "uvrt_create: no HIP device (%s)", hipGetErrorString(e));
    if (device_id < 0 || device_id >= ndev)
        return fail(UVRT_ERR_INVALID, "uvrt_create: device %d out of range [0,%d)", device_id, ndev);
    hipDeviceProp_t prop;
    HIP_TRY(hipGetDeviceProperties(&prop, device_id));
    if (strncmp(prop.gcnArchName, "gfx950", 6) != 0)
        return fail(UVRT_ERR_NO_DEVICE, "uvrt_create: device %d is %s, this library is built for gfx950 only",
                    device_id, prop.gcnArchName);
    std::unique_ptr<uvrt_ctx> c(new uvrt_ctx());      // every error return below destroys what it has made so far
    c->device = device_id;
    c->hot.reserve(uvrt_ctx::HOT_MAX);         // entries are referred to by pointer while their set-up is pending
    c->num_cus = prop.multiProcessorCount > 0 ? prop.multiProcessorCount : 256;
    if (c->num_cus > 256) c->num_cus = 256;   // the overflow-stack buffer is sized for 256 CUs x 16 workgroups
    env_int("UVRT_REPLICAS", 1, 64, c->replicas_knob);   // developer knob: deposit replicas of tempPhotonMap
    HIP_TRY(hipSetDevice(device_id));
    HIP_TRY(hipStreamCreateWithFlags(&c->own_stream, hipStreamNonBlocking));
    c->stream = c->own_stream;
    for (int l = 0; l < uvrt_ctx::MAXL; ++l) {
        if (l > 0) HIP_TRY(hipStreamCreateWithFlags(&c->lanes[l].side, hipStreamNonBlocking));
        HIP_TRY(hipEventCreateWithFlags(&c->lanes[l].ev_tail, hipEventDisableTiming));
    }
    HIP_TRY(hipEventCreateWithFlags(&c->ev_fence, hipEventDisableTiming));
    HIP_TRY(hipEventCreateWithFlags(&c->ev_mapfence, hipEventDisableTiming));
    env_int("UVRT_LANES", 1, uvrt_ctx::MAXL, c->nlanes);
    env_bool("UVRT_PIPELINE", c->pipeline);   // developer knob
    if (long mb = 0; env_int("UVRT_BATCH_CHUNK_MB", 1, LONG_MAX, mb)) c->batch_chunk_bytes = c->dedupe_chunk_bytes = (size_t)mb << 20;
#ifdef UVRT_DEV_VARIANTS
    env_int("UVRT_PROBE_SKIP_GENERATE", INT_MIN, INT_MAX, c->probe_skip_generate);
    env_bool("UVRT_NEARFAR_MINMAX", c->nearfar_minmax);   // the checker / A-B partner of the sign-ordered block
#endif
    env_bool("UVRT_DRAIN_MERGE", c->drain_merge);      // developer knob
    env_bool("UVRT_DEDUPE", c->dedupe);                 // uvrt_set_dedupe's default
    env_int("UVRT_DEDUPE_CLASSES", 0, DEDUPE_CLASS_MAX, c->dedupe_classes);   // uvrt_set_dedupe_classes' default
    env_bool("UVRT_DEDUPE_PERIODIC", c->dedupe_periodic);   // uvrt_set_dedupe_periodic's default
    env_int("UVRT_DEDUPE_STRIP", 1, 1024, c->dedupe_strip);   // developer knob: tiles per wave of the mark pass
    env_int("UVRT_DEDUPE_CLASS_REPLICAS", 1, 16, c->dedupe_class_replicas);
    if (long mb = 0; env_int("UVRT_DEDUPE_CLASS_MB", 1, 4096, mb)) c->dedupe_class_bytes = (size_t)mb << 20;
    env_int("UVRT_HELPER_PRIO", 0, 3, c->helper_prio);   // uvrt_set_helper_priority's default
    env_int("UVRT_BATCH_LANES", 1, uvrt_ctx::MAXL - 1, c->batch_lanes);
    if (int cus = 0; env_int("UVRT_COMM_RESERVE_CUS", 0, 64, cus) && cus % 8 == 0) c->comm_reserve_knob = cus;
    env_int("UVRT_HOT_SAMPLE", 256, 1 << 20, c->hot_sample);
    env_int("UVRT_HOT_DIRECT", 0, 8192, c->hot_direct);
    env_int("UVRT_HOT_TAIL", 0, 63, c->hot_tail);
    if (int rc = c->error_flag.ensure(256, true, c->stream)) return rc;      // (a developer build keeps trip statistics behind the flag)
#ifndef UVRT_TRIP_STATS
    // the stack-overflow flag lives in pinned host memory the kernels can write: uvrt_sync reads it after the stream sync
    // instead of copying a device word back (a pageable 4-byte copy cost every sync ~10 us)
    void* dp = nullptr;
    HIP_TRY(hipHostMalloc((void**)&c->host_flag, 64, hipHostMallocMapped | hipHostMallocCoherent));
    HIP_TRY(hipHostGetDevicePointer(&dp, c->host_flag, 0));
    memset(c->host_flag, 0, 64);
    c->host_flag_dev = (uint32_t*)dp;
#endif
    // lane 0's overflow stack: 256 CUs x 16 workgroups x 256 threads x 24 entries, the largest persistent grid (side lanes
    // get theirs, side_ovf_bytes(), with their first launch)
    if (int rc = c->lanes[0].ovf.ensure((size_t)OVF_MAX_ENTRIES * sizeof(uint32_t), false, c->stream)) return rc;
    *out = c.release();
    return UVRT_OK;
}

void uvrt_destroy(uvrt_ctx* c)
{
    if (!c) return;
    (void)hipSetDevice(c->device);
    // nothing is freed while a stream may still run work that reads it
    (void)hipStreamSynchronize(c->stream);
    for (Lane& L : c->lanes) if (L.side) (void)hipStreamSynchronize(L.side);
    if (c->probe_stream) (void)hipStreamSynchronize(c->probe_stream);
    if (c->comm) uvrt_comm_destroy(c);       // first: it restores the lanes' plain streams
    delete c;
}

int uvrt_set_stream(uvrt_ctx* c, void* hip_stream)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->stream = hip_stream ? (hipStream_t)hip_stream : c->own_stream;
    c->lane = 0;
    return UVRT_OK;
}

int uvrt_set_scene(uvrt_ctx* c, const void* tris64, int32_t T, const void* nodes32,
                   int32_t node_count, const uint32_t* tri_idx)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_set_scene: null argument");
    SceneLayout L;
    std::string why;
    if (int rc = sl::build_scene_layout(tris64, T, nodes32, node_count, tri_idx, L, why)) return fail(rc, "%s", why.c_str());
    if (int rc = set_device(c)) return rc;
    if (int rcj = join_all(c)) return rcj;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->lane = 0;
    if (int rc = provision_scene(c, L, T)) return rc;
    if (int rc = upload_scene(c, L, tris64, T, tri_idx)) return rc;
    return void_scene_state(c);
}

int uvrt_resize_rays(uvrt_ctx* c, int64_t photon_count)
{
    if (!c || photon_count < 0) return fail(UVRT_ERR_INVALID, "uvrt_resize_rays: bad argument");
    if (int rc = set_device(c)) return rc;
    if (photon_count == c->capacity && c->lanes[0].rays.p && (!c->record_hits || c->hits.p)) { c->last = {}; return UVRT_OK; }
    if (int rcj = join_all(c)) return rcj;
    HIP_TRY(hipStreamSynchronize(c->stream));
    c->lane = 0;
    int rc;
    const size_t n = (size_t)photon_count;
    for (int l = 0; l < c->nlanes; ++l)
        if ((rc = c->lanes[l].rays.ensure(n * 16, false, c->stream))) return rc;
    if ((rc = c->keyrank.ensure(n * 8, false, c->stream))) return rc;
    if ((rc = c->sorted.ensure(n * 16, false, c->stream))) return rc;
    if ((rc = c->order.ensure(n * 4, false, c->stream))) return rc;
    if (c->record_hits && (rc = c->hits.ensure(n * 8, false, c->stream))) return rc;
    for (Lane& L : c->lanes) L.oxz.release();         // [capacity]: back with the lane's next free launch
    c->capacity = photon_count;
    c->last = {};
    return UVRT_OK;
}

int uvrt_reset(uvrt_ctx* c, int32_t reset_color)
{
    if (!c || !c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_reset: no scene");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    launch_reset(c->photon_map.as<double>(), c->max_map.as<double>(), c->lanes[0].counts.as<int32_t>(),
                 c->replicas, c->T, c->color.as<float>(), reset_color, c->T, c->helper_prio, c->stream);
    HIP_TRY(hipGetLastError());
    // side-lane count buffers are zero unless an extend was never accumulated; only then must later
    // generate / extend work on the side streams wait for this reset (lane 0's: k_reset)
    bool dirty = false;
    for (int l = 0; l < uvrt_ctx::MAXL; ++l) {
        Lane& L = c->lanes[l];
        if (l > 0 && L.counts_dirty && L.counts.p) {
            HIP_TRY(hipMemsetAsync(L.counts.p, 0, L.counts.bytes, c->stream));
            dirty = true;
        }
        L.counts_dirty = false;
    }
    if (c->b_count > 0) {     // a traced batch that was never replayed: drop its deposits
        if (c->b_is_folded) HIP_TRY(hipMemsetAsync(c->bs[c->b_set].folded.p, 0, c->bs[c->b_set].folded.bytes, c->stream));
        else HIP_TRY(hipMemsetAsync(c->bs[c->b_set].planes.p, 0, c->bs[c->b_set].planes.bytes, c->stream));
        HIP_TRY(hipEventRecord(c->bs[c->b_set].free_ev, c->stream));
        c->b_count = 0;
        c->b_is_folded = false;
    }
    return dirty ? mark_fence(c) : mark_map_fence(c);
}

int uvrt_set_record_perm(uvrt_ctx* c, const uint32_t* perm, int32_t n)
{
    if (!c || !c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_set_record_perm: no scene");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    for (Lane& L : c->lanes) L.recs_tag.valid = false;
    if (!perm) { c->have_perm = false; return UVRT_OK; }
    if (n != c->npairs) return fail(UVRT_ERR_INVALID, "uvrt_set_record_perm: %d entries, the scene has %d inner nodes", n, c->npairs);
    std::vector<uint8_t> seen((size_t)n, 0);
    for (int32_t i = 0; i < n; ++i) {
        if (perm[i] >= (uint32_t)n || seen[perm[i]]) return fail(UVRT_ERR_INVALID, "uvrt_set_record_perm: not a permutation");
        seen[perm[i]] = 1;
    }
    if (n == 0) { c->have_perm = false; return UVRT_OK; }
    if (int rc = c->perm.ensure((size_t)n * 4, false, c->stream)) return rc;
    if (int rc = copy_sync(c, c->perm.p, perm, (size_t)n * 4, hipMemcpyHostToDevice)) return rc;
    c->have_perm = true;
    c->perm_gen = ++c->perm_clock;       // same address, another renumbering: records prepared from the old one are stale
    return UVRT_OK;
}

int uvrt_read_record_perm(uvrt_ctx* c, uint32_t* out, int32_t n)
{
    if (!c || !out || !c->have_scene || n != c->npairs)
        return fail(UVRT_ERR_INVALID, "uvrt_read_record_perm: need a scene and n = its %d inner nodes", c ? c->npairs : 0);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    const uint32_t* pm = c->have_perm ? c->perm.as<uint32_t>() : cur_lane(c).perm;
    if (!pm) { for (int32_t i = 0; i < n; ++i) out[i] = (uint32_t)i; return UVRT_OK; }
    return copy_sync(c, out, pm, (size_t)n * 4, hipMemcpyDeviceToHost);
}

int uvrt_sync(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    uint32_t flag = 0;
#ifdef UVRT_TRIP_STATS
    HIP_TRY(hipMemcpyAsync(&flag, c->error_flag.p, 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
#else
    HIP_TRY(hipStreamSynchronize(c->stream));
    flag = *(volatile uint32_t*)c->host_flag;
#endif
#ifdef UVRT_TRIP_STATS
    if (getenv("UVRT_TRIP_STATS")) {
        unsigned long long st[27];
        HIP_TRY(hipMemcpy(st, (char*)c->error_flag.p + 8, sizeof st, hipMemcpyDeviceToHost));
        HIP_TRY(hipMemset((char*)c->error_flag.p + 8, 0, sizeof st));
        if (st[1]) {
            const double t = (double)st[1];
            fprintf(stderr, "trip stats: waves %llu trips %llu (%.1f per wave)  lanes per trip: inner %.2f leaf-visit %.2f leaf-wait %.2f "
                    "idle %.2f  cached %.2f  leaf trips %.3f  drain trips %.3f  slow trips %.4f (sp>=9 %.4f >=10 %.4f >=11 %.4f >=12 %.4f)  "
                    "refills/wave %.1f\n",
                    st[0], st[1], t / (double)st[0], st[2] / t, st[3] / t, st[4] / t, st[5] / t, st[10] / t, st[6] / t, st[7] / t,
                    st[8] / t, st[11] / t, st[12] / t, st[13] / t, st[14] / t, (double)st[9] / (double)st[0]);
            const double w = (double)st[0];
            fprintf(stderr, "trip clocks (s_memtime ticks per wave): life %.0f  record fetch %.0f  leaf tests %.0f  box tests + descend %.0f  "
                    "refill %.0f  general step %.0f  rest (loop overhead) %.0f;  per trip: fetch %.0f leaf %.0f box %.0f; per refill %.0f; per general step %.0f\n",
                    st[19] / w, st[15] / w, st[16] / w, st[17] / w, st[18] / w, st[20] / w,
                    (st[19] - st[15] - st[16] - st[17] - st[18] - st[20]) / w,
                    st[15] / t, st[16] / t, st[17] / t, (double)st[18] / (double)(st[9] ? st[9] : 1), (double)st[20] / (double)(st[8] ? st[8] : 1));
            // totals since the last sync, for tests/tools/stream_census.py
            fprintf(stderr, "trip census: waves %llu stream_in %llu stream_leaf %llu stream_both %llu general_exact %llu general_other %llu "
                    "refills %llu leaf_lane_tests %llu trips %llu\n", st[0], st[21], st[22], st[23], st[24], st[25], st[9], st[26], st[1]);
        }
    }
#endif
    if (flag) {
#ifdef UVRT_TRIP_STATS
        HIP_TRY(hipMemsetAsync(c->error_flag.p, 0, 4, c->stream));
#else
        *(volatile uint32_t*)c->host_flag = 0u;
#endif
        return fail(UVRT_ERR_STACK, "extend: BVH traversal needed more than 32 stack entries (extend.cl:43)");
    }
    return UVRT_OK;
}

// a range of one of the context's per-triangle arrays
static int read_back(uvrt_ctx* c, const DevBuf* b, size_t elem, void* out, int64_t first, int64_t count, const char* what)
{
    const int64_t limit = c ? c->T : 0;
    if (!c || !range_ok(out, first, count, limit))
        return fail(UVRT_ERR_INVALID, "%s: range [%lld,+%lld) outside [0,%lld)", what, (long long)first,
                    (long long)count, (long long)limit);
    return range_copy(c, b->p, elem, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_read_dosage(uvrt_ctx* c, float* out, int32_t first, int32_t count)
{
    return read_back(c, c ? &c->dosage : nullptr, 4, out, first, count, "uvrt_read_dosage");
}
int uvrt_read_color(uvrt_ctx* c, float* out9, int32_t first, int32_t count)
{
    return read_back(c, c ? &c->color : nullptr, 36, out9, first, count, "uvrt_read_color");
}
int uvrt_read_counts(uvrt_ctx* c, int32_t* out, int32_t first, int32_t count)
{
    if (c && c->have_scene) {
        if (int rc = set_device(c)) return rc;
        if (int rc = join_all(c)) return rc;
        launch_fold_counts(cur_lane(c).counts.as<int32_t>(), c->replicas, c->T, c->T, c->stream);
        if (int rc = mark_fence(c)) return rc;
    }
    return read_back(c, c ? &cur_lane(c).counts : nullptr, 4, out, first, count, "uvrt_read_counts");
}
int uvrt_read_photon_map(uvrt_ctx* c, int32_t which, double* out, int32_t first, int32_t count)
{
    if (which != UVRT_MAP_SUM && which != UVRT_MAP_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_read_photon_map: which_map must be 0 or 1");
    return read_back(c, c ? (which == UVRT_MAP_SUM ? &c->photon_map : &c->max_map) : nullptr, 8, out, first,
                     count, "uvrt_read_photon_map");
}

int uvrt_get_seed(uvrt_ctx* c, uint32_t* seed)
{
    if (!c || !seed) return fail(UVRT_ERR_INVALID, "null argument");
    *seed = c->seed;
    return UVRT_OK;
}
int uvrt_set_seed(uvrt_ctx* c, uint32_t seed)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    c->seed = seed;
    return UVRT_OK;
}

int uvrt_set_wide_bvh(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    c->wide = on != 0;
    return UVRT_OK;
}

int uvrt_set_hot_records(uvrt_ctx* c, int32_t mode)
{
    if (!c || (mode != 0 && mode != 1)) return fail(UVRT_ERR_INVALID, "uvrt_set_hot_records: mode must be 0 or 1");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    c->hot_mode = mode;
    for (Lane& L : c->lanes) { L.recs_tag.valid = false; L.perm = nullptr; }
    return UVRT_OK;
}

int uvrt_set_dedupe(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    c->dedupe = on != 0;
    return UVRT_OK;
}

int uvrt_set_dedupe_classes(uvrt_ctx* c, int32_t max_classes)
{
    if (!c || max_classes < 0 || max_classes > DEDUPE_CLASS_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_set_dedupe_classes: the maximum must be 0..%d", DEDUPE_CLASS_MAX);
    c->dedupe_classes = max_classes;
    return UVRT_OK;
}

int uvrt_get_dedupe_classes(uvrt_ctx* c, int32_t* max_classes)
{
    if (!c || !max_classes) return fail(UVRT_ERR_INVALID, "uvrt_get_dedupe_classes: null argument");
    *max_classes = c->dedupe_classes;
    return UVRT_OK;
}

int uvrt_set_dedupe_periodic(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_set_dedupe_periodic: null context");
    c->dedupe_periodic = on != 0;
    return UVRT_OK;
}

int uvrt_get_dedupe_periodic(uvrt_ctx* c, int32_t* on)
{
    if (!c || !on) return fail(UVRT_ERR_INVALID, "uvrt_get_dedupe_periodic: null argument");
    *on = c->dedupe_periodic ? 1 : 0;
    return UVRT_OK;
}

int uvrt_set_helper_priority(uvrt_ctx* c, int32_t prio)
{
    if (!c || prio < 0 || prio > 3) return fail(UVRT_ERR_INVALID, "uvrt_set_helper_priority: the level must be 0..3");
    c->helper_prio = prio;
    return UVRT_OK;
}

int uvrt_get_helper_priority(uvrt_ctx* c, int32_t* prio)
{
    if (!c || !prio) return fail(UVRT_ERR_INVALID, "uvrt_get_helper_priority: null argument");
    *prio = c->helper_prio;
    return UVRT_OK;
}

int uvrt_set_seed_mode(uvrt_ctx* c, int32_t mode)
{
    if (!c || (mode != 0 && mode != 1)) return fail(UVRT_ERR_INVALID, "uvrt_set_seed_mode: mode must be 0 or 1");
    c->seed_mode = mode;
    return UVRT_OK;
}

int uvrt_set_sort_bits(uvrt_ctx* c, int32_t bits)
{
    if (!c || bits < -1 || bits > 20) return fail(UVRT_ERR_INVALID, "uvrt_set_sort_bits: bits must be in [-1,20]");
    c->sort_bits = bits;
    return UVRT_OK;
}
int uvrt_set_record_hits(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    c->record_hits = on != 0;
    return UVRT_OK;
}
int uvrt_set_flavour(uvrt_ctx* c, int32_t flavour)
{
    if (!c || flavour < 0 || flavour > 2) return fail(UVRT_ERR_INVALID, "uvrt_set_flavour: flavour must be 0, 1 or 2");
    c->flavour = flavour;
    return UVRT_OK;
}
int uvrt_set_variant(uvrt_ctx* c, int32_t variant)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    if (!variant_ok(variant))
        return fail(UVRT_ERR_INVALID, "uvrt_set_variant: %d is not a variant of this build (0, 400-1299; codes other than 1 in the "
                    "last digit need the developer build libuvrt_hip_dev.so)", variant);
    c->variant = variant;
    return UVRT_OK;
}
int uvrt_set_pipeline(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    c->pipeline = on != 0;
    return UVRT_OK;
}
int uvrt_set_timing(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "null context");
    c->timing = on != 0;
    return UVRT_OK;
}

int uvrt_read_rays(uvrt_ctx* c, void* rays32, int64_t first, int64_t count)
{
    if (!c || !rays32 || c->last.n < 0 || first < 0 || count < 0 || first + count > c->last.n)
        return fail(UVRT_ERR_INVALID, "uvrt_read_rays: range outside the last generate");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    if (count == 0) return UVRT_OK;
    if (int rc = c->export_buf.ensure((size_t)count * 32, false, c->stream)) return rc;
    const uint2* hits = (c->last.extended && c->hits.p) ? c->hits.as<uint2>() : nullptr;
    if (c->last.free_rays)
        launch_export_free_rays(cur_lane(c).rays.as<float4>(), cur_lane(c).oxz.as<float2>(), hits, c->export_buf.p, first, count, c->stream);
    else
        launch_export_rays(cur_lane(c).rays.as<float4>(), hits, c->export_buf.p, c->ox, c->oz, first, count, c->stream);
    HIP_TRY(hipGetLastError());
    return copy_sync(c, rays32, c->export_buf.p, (size_t)count * 32, hipMemcpyDeviceToHost);
}

int uvrt_write_rays(uvrt_ctx* c, const void* rays32, int64_t n)
{
    if (!c || !rays32 || n <= 0 || n > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_write_rays: n must be in (0, capacity]");
    if (int rc = set_device(c)) return rc;
    const HostRay* hr = (const HostRay*)rays32;
    for (int64_t i = 0; i < n; ++i)
        if (memcmp(&hr[i].o[0], &hr[0].o[0], 4) != 0 || memcmp(&hr[i].o[2], &hr[0].o[2], 4) != 0)
            return fail(UVRT_ERR_INVALID, "uvrt_write_rays: record %lld has a different orig.x/orig.z", (long long)i);
    std::vector<float> packed;
    unpack_rays(hr, n, packed);
    if (int rc = join_all(c)) return rc;
    c->lane = 0;
    c->cur_pipelined = false;
    Lane& L = c->lanes[0];
    if (int rc = copy_sync(c, L.rays.p, packed.data(), (size_t)n * 16, hipMemcpyHostToDevice)) return rc;
    L.recs_tag.valid = false;
    L.perm = nullptr;
    c->last = {n, 0, false, false, false};
    c->ox = hr[0].o[0];
    c->oz = hr[0].o[2];
    return UVRT_OK;
}

int uvrt_device_ptr(uvrt_ctx* c, int32_t which, void** ptr, int64_t* bytes)
{
    if (!c || !ptr || !bytes || !c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_device_ptr: bad argument");
    // the caller is about to touch the buffers on the context's stream: order it after the side lane,
    // and the side lane's next work after whatever the caller enqueues up to the next call
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    const DevBuf* b = nullptr;
    size_t elem = 0;
    switch (which) {
        case 0: b = &c->photon_map; elem = 8; break;
        case 1: b = &c->max_map; elem = 8; break;
        case 2:
            b = &cur_lane(c).counts; elem = 4;
            launch_fold_counts(b->as<int32_t>(), c->replicas, c->T, c->T, c->stream);
            break;
        case 3: b = &c->dosage; elem = 4; break;
        case 4: b = &c->color; elem = 36; break;
        case 5:
            if (c->b_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_device_ptr: no traced batch");
            if (int rc = uvrt_fold_batch(c)) return rc;
            b = &c->bs[c->b_set].folded; elem = 4 * (size_t)c->b_count;
            break;
        case 6:
            if (int rc = ensure_expected(c)) return rc;
            b = &c->derived.expected; elem = 8;
            break;
        case 7:
            if (int rc = ensure_variance(c)) return rc;
            b = &c->derived.variance; elem = 8;
            break;
        case 8:
            if (int rc = ensure_source(c)) return rc;
            b = &c->derived.source; elem = 8;
            break;
        default: return fail(UVRT_ERR_INVALID, "uvrt_device_ptr: which must be 0..8");
    }
    *ptr = b->p;
    *bytes = (int64_t)((size_t)c->T * elem);
    // see lane_stream(): the next side-lane work (on the maps: the next accumulate / Shade) waits for
    // what the caller enqueues on the main stream up to the next call
    // (the folded planes of a batch are only touched on the context's stream until their replay: no fence)
    if (which == 2) c->ext_touch = true; else if (which != 5) c->ext_touch_maps = true;
    return UVRT_OK;
}

int uvrt_copy_device(uvrt_ctx* c, int32_t which, void* ext, int32_t to_ctx)
{
    void* p = nullptr;
    int64_t bytes = 0;
    if (!ext) return fail(UVRT_ERR_INVALID, "uvrt_copy_device: null pointer");
    if (int rc = uvrt_device_ptr(c, which, &p, &bytes)) return rc;
    if (int rc = set_device(c)) return rc;
    if (to_ctx) HIP_TRY(hipMemcpyAsync(p, ext, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream));
    else HIP_TRY(hipMemcpyAsync(ext, p, (size_t)bytes, hipMemcpyDeviceToDevice, c->stream));
    return mark_fence(c);
}

int uvrt_extend_time_ms(uvrt_ctx* c, double* ms, int64_t* launches)
{
    if (!c || !ms || !launches) return fail(UVRT_ERR_INVALID, "null argument");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    double total = 0;
    for (size_t i = 0; i < c->ev_used; ++i) {
        float t = 0;
        HIP_TRY(hipEventElapsedTime(&t, c->ev_pool[2 * i], c->ev_pool[2 * i + 1]));
        total += t;
    }
    *ms = total;
    *launches = (int64_t)c->ev_used;
    c->ev_used = 0;
    return UVRT_OK;
}

}  // extern "C"

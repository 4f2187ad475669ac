// uvrt_ctx.h -- the context behind the C ABI of include/uvrt.h, shared by the translation units that implement it:
//   uvrt_capi.hip         context, scene, buffers, knobs, read-backs and test hooks; the scene is provisioned and uploaded from
//   uvrt_scene_layout.h   the host-only re-layout of a scene (build_scene_layout): no HIP, testable alone
//   uvrt_capi_launch.hip  the per-launch entry points (generate, extend, accumulate, shade) and the launch lanes
//   uvrt_capi_batch.hip   batched tracing (uvrt_trace_batch / uvrt_trace_batch_launches / fold / replay): provisioning, the
//                         chunk emitters and the commit, over the plan of
//   uvrt_batch_plan.h     the host-only plan of a batch (plan_batch, deal_classes, mark_tiles): no HIP, testable alone
//   uvrt_capi_free.hip    rays with origins of their own (uvrt_write_free_rays, uvrt_generate_sweep)
//   uvrt_capi_gather.hip  shadow rays and the direct gather (uvrt_occluded, uvrt_gather_direct, uvrt_accumulate_expected,
//                         uvrt_set_gather_variance and the variance plane, uvrt_set_gather_faces and the face planes,
//                         uvrt_gather_refine)
//   uvrt_capi_gather_batch.hip  the batched direct gather (uvrt_gather_direct_batch, uvrt_gather_batch_select)
//   uvrt_capi_indirect.hip  closest hits and the one-bounce gather (uvrt_closest_hits, uvrt_gather_indirect, the source plane)
//   uvrt_capi_links.hip   recorded hit links and the multi-bounce gather over them (uvrt_indirect_links_build,
//                         uvrt_gather_indirect_linked) and their sided forms (uvrt_indirect_links_build_sided,
//                         uvrt_gather_indirect_linked_sided)
//   uvrt_capi_mirror.hip  specular panels and the mirror gather (uvrt_set_mirrors, uvrt_gather_mirror)
//   uvrt_capi_sensors.hip virtual dosimeters (uvrt_set_sensors, uvrt_gather_sensors, uvrt_gather_sensors_indirect and the
//                         sensors' own planes)
//   uvrt_capi_comm.hip    the one collective of a sharded computation (RCCL, opened at run time)
//
// One context = one HIP device + one in-order stream + all device buffers of a RayTracer
// (raytracer.h:50-53), its per-launch state split over launch lanes (struct Lane).
// There is no CPU fallback: every entry point either runs on the GPU or returns an error.
//
// Who owns what.  A DevBuf owns its allocation, a Lane its side stream and tail event, a BatchSet its free event, the
// context the rest (~uvrt_ctx).  A member added to one of these structs is released with it: there is no list to extend.
// Buffers are named for release only where a SUBSET is dropped on purpose, per capacity (uvrt_resize_rays) or per scene.
// Per scene (uvrt_capi.hip void_scene_state): what is derived from the scene and made on first use lives in
// uvrt_ctx::SceneDerived and is dropped whole, so a member added there is voided with it; named beside it are only the few
// that need handling of their own -- the lanes' record tags and recs4, the caller's renumbering, the hot entries
// (hot_reset), the plan (plan_drop) and the traced batch.
// Destruction order.  No destructor waits for a stream, so nothing may be deleted while a stream can still run work that
// reads it: uvrt_destroy makes the device current, waits for the context's stream, the side streams and the probe's,
// destroys the communicator (which puts the lanes' plain streams back) and only then deletes the context.  plan_drop waits
// for the context's stream itself: it also runs in the middle of a context's life.
#pragma once
#include "../../include/uvrt.h"
#include "uvrt_device.h"
#include "uvrt_batch_plan.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

namespace uvrt_impl {

extern thread_local std::string g_err;      // uvrt_last_error()
int fail(int code, const char* fmt, ...);   // sets g_err, returns code

#define HIP_TRY(expr)                                                                   \
    do {                                                                                \
        hipError_t e_ = (expr);                                                         \
        if (e_ != hipSuccess)                                                           \
            return ::uvrt_impl::fail(UVRT_ERR_HIP, "%s failed: %s (%s:%d)", #expr,      \
                                     hipGetErrorString(e_), __FILE__, __LINE__);        \
    } while (0)

// A device allocation and its owner: move-only, freed by its destructor (so a struct of them needs no release list).
struct DevBuf {
    void* p = nullptr;
    size_t bytes = 0;
    DevBuf() = default;
    DevBuf(DevBuf&& o) noexcept : p(o.p), bytes(o.bytes) { o.p = nullptr; o.bytes = 0; }
    DevBuf& operator=(DevBuf&& o) noexcept
    {
        if (this != &o) { release(); p = o.p; bytes = o.bytes; o.p = nullptr; o.bytes = 0; }
        return *this;
    }
    ~DevBuf() { release(); }
    // Zeroing is enqueued on `s`, the stream every kernel of the context runs on (the
    // context's stream is non-blocking, so a null-stream hipMemset would not be ordered
    // against it).
    int ensure(size_t need, bool zero, hipStream_t s)
    {
        if (need <= bytes && p) return UVRT_OK;
        if (p) { HIP_TRY(hipFree(p)); p = nullptr; bytes = 0; }
        if (need == 0) return UVRT_OK;
        HIP_TRY(hipMalloc(&p, need));
        bytes = need;
        if (zero) HIP_TRY(hipMemsetAsync(p, 0, need, s));
        return UVRT_OK;
    }
    void release() { if (p) (void)hipFree(p); p = nullptr; bytes = 0; }
    template <class T> T* as() const { return (T*)p; }
};

// What an array of per-launch records is prepared for: the lamp column (ox, oz).  Compared bitwise, so that
// -0.0f and 0.0f are different columns.
struct RecsTag {
    bool valid = false;
    float ox = 0, oz = 0;
    bool matches(float x, float z) const { return valid && memcmp(&ox, &x, 4) == 0 && memcmp(&oz, &z, 4) == 0; }
};

// A launch lane: a stream with its own ray, record, count and overflow-stack buffers.
// Lane 0 runs on the context's stream, which uvrt_set_stream may replace: stream_of() is the one place that knows it.
struct Lane {
    hipStream_t side = nullptr;      // the lane's own stream (lanes 1..MAXL-1; null for lane 0)
    hipEvent_t ev_tail = nullptr;    // tail of the lane's stream
    bool used = false;               // the side stream holds work the main stream is not ordered after
    uint64_t seen_fence = 0, seen_mapfence = 0;   // the last fence / map fence the side stream waits for
    DevBuf rays, recs, counts;       // rays of the launch; records [0, npairs) per launch + leaf records; replicas x T deposits
    DevBuf ovf;                      // traversal-stack entries 8..31 of every thread of the persistent grid
    RecsTag recs_tag;                // what recs[0, npairs) is prepared for
    bool counts_dirty = false;       // `counts` holds deposits that were not accumulated
    DevBuf recs4;                    // 4-wide walk: [2 * nquads + T + 1] 64-byte units, per-launch form + leaf records
    RecsTag recs4_tag;               // what the per-launch part of recs4 is prepared for
    DevBuf hot_hist, hot_list;       // scratch of the hot-record set-up kernels (uvrt_hotset.hip)
    const uint32_t* perm = nullptr;  // renumbering of the lane's current launch (set by uvrt_generate)
    DevBuf oxz;                      // {orig.x, orig.z} of free rays, [capacity]; allocated by the lane's first free launch
    DevBuf dd_tmp, dd_blocks;        // a deduped chunk's scratch between the passes of its generate (GenDedupeParams tmp, block_counts;
                                     // dd_blocks is allocated zeroed and every chunk leaves it zero)
    ~Lane() { if (ev_tail) (void)hipEventDestroy(ev_tail); if (side) (void)hipStreamDestroy(side); }
};

}  // namespace uvrt_impl

using uvrt_impl::DevBuf;
using uvrt_impl::Lane;
using uvrt_impl::RecsTag;

struct uvrt_ctx {
    int device = 0;
    int num_cus = 256;
    hipStream_t own_stream = nullptr;
    hipStream_t stream = nullptr;

    // scene
    int32_t T = 0;
    DevBuf pairs, perm, ltris, leaf_count, area;
    bool have_perm = false;      // the caller's own record renumbering (uvrt_set_record_perm)
    uint64_t perm_clock = 0;     // stamps every renumbering written into `perm` or a hot entry
    uint64_t perm_gen = 0;       // stamp of what `perm` holds
    int32_t npairs = 0;
    uint32_t root_ref = uvrt::REF_DONE;
    uint32_t top_pairs = 0;      // inner nodes at tree depths 0..7, the first eight levels, TOP6_MAX at most (breadth-first prefix of `pairs`)
    bool have_scene = false;
    int32_t replicas = 1;        // deposit replicas of tempPhotonMap (uvrt_device.h ExtendParams)
    int32_t replicas_knob = -1;  // -1: choose from T

    // per-triangle maps (raytracer.cpp:32-37)
    DevBuf photon_map, max_map, dosage, color;

    // rays (the launch's own rays are per launch lane)
    int64_t capacity = 0;
    DevBuf keyrank, sorted, order, hits, hist, bin_start, export_buf;
    bool drain_merge = true;                   // k_extend6's workgroups pool the last rays of their waves (ExtendParams::drain_merge; developer knob UVRT_DRAIN_MERGE=0)
    bool nearfar_minmax = false;               // developer build: k_extend6's stream with the min/max near / far block (ExtendParams::nearfar_minmax; UVRT_NEARFAR_MINMAX=1)
    bool scene_force_exact = false;            // a node bound too tiny / too large for the reciprocal shortcuts
    int32_t hist_bins = 0;
    // the rays of the last generate (or write): what uvrt_extend and uvrt_read_rays work on (n = -1: none; free_rays: with
    // origins of their own, uvrt_capi_free.hip).  Assigned whole.
    struct LastRays { int64_t n = -1, first = 0; bool sorted = false, extended = false, free_rays = false; } last;
    float ox = 0, oz = 0;
    // shadow rays and the direct gather (uvrt_capi_gather.hip): every ray's {orig.x, orig.z}, tmax and answer and the samples'
    // weights, made on first use.  (The rays themselves go through lane 0's ray buffer, on the context's stream.)
    DevBuf g_oxz, g_tmax, g_occ, g_w;
    DevBuf g_face;                             // the face each sample arrives on, uint8[capacity] (uvrt_set_gather_faces)
    DevBuf g_hit;                              // closest hits (uvrt_capi_indirect.hip): every ray's (dist bits, triID), uint2[capacity]
    DevBuf g_point;                            // the mirror gather's receiver points (uvrt_capi_mirror.hip), float4[capacity]
    // virtual dosimeters (uvrt_capi_sensors.hip): the context's, not the scene's, so uvrt_set_scene leaves them alone.  The
    // caller's records as they came (host and device), the five planes f64[5][K] and the dosage read-back's f32[K];
    // sensor_count 0: none
    int32_t sensor_count = 0;
    std::vector<uvrt_sensor> sensors;
    DevBuf sensors_dev, sensor_planes, sensor_out;
    // uvrt_gather_refine (include/uvrt.h "adaptive gather"): the exclusive prefix sums of a refined range, int32[T + 1], and
    // the scan's per-block totals
    DevBuf g_offs, g_scan;
    // the last successful uvrt_gather_direct with the variance plane on: what uvrt_gather_refine refines.  Host state only.
    // Assigned whole; `valid` false: forgotten.
    struct GatherMemo {
        bool valid = false;
        int32_t first = 0, count = 0, samples = 0, mode = 0, photons_equiv = 0;
        uint32_t seed = 0;
        float from[3] = {0, 0, 0}, to[3] = {0, 0, 0}, light_length = 0;
    };
    // What is derived from the scene and made on first use.  uvrt_set_scene drops the struct whole (void_scene_state,
    // uvrt_capi.hip): a member added here is voided with it.
    struct SceneDerived {
        DevBuf free_recs;                      // the free-origin kernel's records, [npairs + T + 1] x 64 B
        bool free_recs_valid = false;          // ... for the current scene
        DevBuf g_tris;                         // the gather's triangles by original id
        bool g_tris_valid = false;             // g_tris holds the current scene
        DevBuf expected, variance;             // the gather's expected plane f64[T] and the variance plane f64[T] beside it
        DevBuf faces;                          // the direct gather's face planes f64[2][T] (made zeroed; uvrt_set_gather_faces)
        DevBuf g_extra;                        // n_t of the last refine, int32[T] (made zeroed)
        DevBuf source;                         // the one-bounce gather's source plane f64[T] (made zeroed)
        // recorded hit links (uvrt_capi_links.hip): int32[links_samples * T], sample-major (links[s * T + t]); links_samples 0:
        // none.  Beside them the linked gather's two irradiance planes (ping-pong over the bounces) and its running total, f64[T]
        DevBuf links, link_e[2], link_total;
        int32_t links_samples = 0, links_flavour = 0;
        int32_t links_kind = 0;                // 0: plain links (h or -1); 1: sided ((h << 1) | arrival face, or -1)
        uint32_t links_seed = 0;
        DevBuf rho;                            // the reflectance planes f32[2][T] of uvrt_gather_indirect_linked_mapped
        bool have_rho = false;                 // ... exist (a scene has none until a fill or a write makes them)
        // specular panels (uvrt_capi_mirror.hip): the caller's records as they came, the planes as the kernels read them
        // (point and unit normal in f64) and panel_of_tri, uint8[T], on the device; mirror_count 0: none
        int32_t mirror_count = 0, mirror_members = 0;
        uvrt_mirror mirrors[UVRT_MIRROR_MAX] = {};
        uvrt::MirrorPanel mirror_planes[UVRT_MIRROR_MAX] = {};
        DevBuf panel_of_tri_dev;
        GatherMemo gather_memo;                // a refine works on one scene's planes
        // the batch of the last successful uvrt_gather_direct_batch (uvrt_capi_gather_batch.hip; count 0: none): its launches,
        // range and sample count, the sampling mode, variance state and flavour it ran under, and its planes f64[count][T]
        // (v: with the variance state on)
        struct GatherBatch {
            int32_t count = 0, samples = 0, first = 0, tri_count = 0, mode = 0, flavour = 0;
            bool var = false;
            std::vector<uvrt_gather_params> launches;
            DevBuf e, v;
        } gather_batch;
    } derived;
    // uvrt_gather_direct_batch's launch table: the host copy the call fills and the device copy it uploads on the stream
    std::vector<uvrt::GatherBatchLaunch> gb_host;
    DevBuf gb_table;

    // Launch lanes: consecutive launches (generate -> extend -> accumulate ->
    // shade) alternate between the context's stream and an internal side stream, each with its own
    // ray, record, count and overflow-stack buffers, so that the next launch fills the wave slots the
    // draining launch frees.  The per-triangle maps are updated in launch order (event waits).
    static constexpr int MAXL = 4;
    Lane lanes[MAXL];                 // lane 0 runs on the context's stream, lanes 1.. on their side streams
    bool pipeline = true;             // uvrt_set_pipeline
    int nlanes = 2;                   // developer knob UVRT_LANES (1..MAXL): 3 gain ~1 %, 4 (with 4 workgroups
                                      // per CU) win only for long launch sequences (profiles/r01/r01_v6_experiments.txt)
    bool ext_touch = false;           // a count-buffer pointer was handed out since the last fence
    bool ext_touch_maps = false;      // a map / dose / colour pointer was handed out since the last map fence
    hipEvent_t ev_mapfence = nullptr; // on the main stream, after the last operation on the per-triangle maps
    uint64_t mapfence_seq = 0;
    int lane = 0;                     // lane of the current launch (uvrt_generate selects it)
    int prev_lane = 0;                // lane of the launch before it (the maps are updated in launch order)
    bool cur_pipelined = false;       // the current launch takes part in the lane rotation
    hipEvent_t ev_fence = nullptr;    // on the main stream, after the last context-wide operation
    uint64_t fence_seq = 0;

    // Opt-in 4-wide collapse of the BVH (uvrt_set_wide_bvh, uvrt_extend4.hip; per-launch records in Lane::recs4)
    bool wide = false;
    DevBuf quads;                         // [nquads] QuadRec, scene form
    int32_t nquads = 0;
    uint32_t top_quads = 0;

    // Hot-record renumbering per lamp position (uvrt_hotset.hip): the records a lamp's photons visit most are
    // the ones the traversal serves from LDS.  Built on the device the first time a lamp is seen.
    // The renumberings live in slabs of HOT_SLAB entries (the first one allocated with the scene, so that a new lamp
    // costs no allocation); the visit counters and the hot list are scratch of the three set-up kernels, one set per
    // launch lane (Lane::hot_hist, hot_list: the kernels of one lamp run back to back on one stream and leave the
    // counters zeroed).
    static constexpr int HOT_SLAB = 16, HOT_MAX = 64;
    struct HotEntry { float lamp[3]; uint32_t* perm; uint64_t stamp; hipEvent_t ready; uint64_t gen; };
    std::vector<HotEntry> hot;
    std::vector<DevBuf> hot_slabs;        // [ceil(entries / HOT_SLAB)]: HOT_SLAB x npairs uint32 each
    int32_t hot_sample = 32768;           // photons of the launch whose visits are counted (developer knob UVRT_HOT_SAMPLE)
    int32_t hot_direct = 8192;            // records k_select_hot takes as candidates without a tree walk (developer knob UVRT_HOT_DIRECT; tests force the walk with it)
    int32_t hot_tail = 16;                // straggler rule of k_visit_stats (developer knob UVRT_HOT_TAIL, uvrt_hotset.hip)
    uint64_t hot_clock = 0;
    int32_t hot_mode = 1;                 // uvrt_set_hot_records: 1 = automatic (default), 0 = breadth-first order

    // Batched tracing (uvrt_trace_batch): the rays of up to MAX_BATCH launches side by side, one count
    // "plane" (replicas x T ints) per launch, one per-launch record array per distinct lamp.
    // two buffer sets: batch k + 1 is traced (on the launch lanes) into one while batch k is folded, reduced and
    // replayed (on the context's stream) out of the other
    // (oxz: the {orig.x, orig.z} of the batch's sweeps, [sweep][n_pad]; allocated by the first batch that holds one)
    // (masks: the planes of every ray of a deduped chunk, indexed like rays; dd_counts: the rays each such chunk holds, uint32 each)
    struct BatchSet { DevBuf rays, planes, folded, oxz, masks, dd_counts; hipEvent_t free_ev = nullptr; ~BatchSet() { if (free_ev) (void)hipEventDestroy(free_ev); } };
    BatchSet bs[2];
    int b_set = 0;                        // the set of the traced batch (b_count > 0) / of the last one
    uint64_t b_chunks = 0;                // chunks traced so far: consecutive chunks alternate over the launch lanes
    int batch_lanes = 2;                  // side lanes the chunks of a batch alternate over (developer knob UVRT_BATCH_LANES: 1..3)
    int32_t b_repl = 16;                  // deposit replicas per plane of the traced batch
    std::vector<DevBuf> b_recs;           // [group]
    // `gen` tells two renumberings apart that live at ONE address: the caller's buffer after another
    // uvrt_set_record_perm, a hot entry recycled for another lamp (perm_clock stamps every (re)written renumbering)
    struct RecsKey {
        RecsTag tag; const uint32_t* perm = nullptr; uint64_t gen = 0;
        bool holds(float ox, float oz, const uint32_t* pm, uint64_t g) const { return tag.matches(ox, oz) && perm == pm && gen == g; }
    };
    std::vector<RecsKey> b_recs_key;      // what b_recs[g] holds
    int32_t b_count = 0;                  // launches of the batch that has not been replayed (0: none)
    int64_t b_n = 0, b_npad = 0;
    int32_t b_phys[uvrt::MAX_BATCH] = {};       // logical launch -> physical plane (launches are grouped by lamp)
    int helper_prio = 1;                  // uvrt_set_helper_priority / UVRT_HELPER_PRIO: s_setprio level (0..3) of the short kernels that run
                                          // beside a traversal grid (uvrt_device.h helper_priority); read at every launch
    bool dedupe = true;                   // uvrt_set_dedupe / UVRT_DEDUPE: a lamp's distinct rays are traced once per batch (uvrt_dedupe.h)
    int64_t b_traced_known = -1;          // uvrt_batch_traced_rays: the last traced batch's rays in chunks traced as they are ...
    int32_t dedupe_strip = 0;             // tiles per wave of the mark pass (developer knob UVRT_DEDUPE_STRIP; 0: uvrt_batch_plan.h mark_tiles)
    int32_t b_traced_chunks = 0;          // ... and its deduped chunks, whose counts are bs[b_set].dd_counts[0, b_traced_chunks)
    // mask classes of a batch's dedupe groups (uvrt_dedupe.h "mask classes")
    int32_t dedupe_classes = uvrt::DEDUPE_CLASSES_DEFAULT;     // uvrt_set_dedupe_classes / UVRT_DEDUPE_CLASSES: classes per group at most, 0 = none
    bool dedupe_periodic = uvrt::DEDUPE_PERIODIC_DEFAULT;      // uvrt_set_dedupe_periodic / UVRT_DEDUPE_PERIODIC: interior masks from the period table (uvrt_dedupe.h)
    int32_t dedupe_class_replicas = 4;    // replicas of a class plane that take deposits (developer knob UVRT_DEDUPE_CLASS_REPLICAS)
    size_t dedupe_class_bytes = (size_t)96 << 20;         // class planes of one buffer set (developer knob UVRT_DEDUPE_CLASS_MB)
    int32_t b_ncls = 0, b_cls_repl = 1;   // the traced batch's class planes (behind its b_count launch planes) and their replicas in use
    uint64_t b_cls_launches[uvrt::MAX_CLASS_PLANES] = {};        // the physical planes each of them is added to
    // (the deduped chunks' deposit counts follow their ray counts in dd_counts: uvrt_batch_deposits)
    bool b_is_folded = false;             // b_folded holds the batch (fold / all-reduce done), the replicas are zero
    void* comm = nullptr;                 // ncclComm_t of a ray-range-sharded job (uvrt_comm_init_rank)
    // CUs the launch lanes leave to the context's stream while a communicator is set (uvrt_capi_comm.hip
    // reserve_cus_for_comm): the lanes' streams carry a CU mask, the persistent grids are sized for the rest
    int comm_reserve_knob = 8;            // developer knob UVRT_COMM_RESERVE_CUS (a multiple of 8, 0 = none)
    int lanes_masked_cus = 0;             // CUs masked out of the side lanes' streams right now
    int comm_rank = 0, comm_world = 1;

    // generate.cl:6 program-scope SEED
    uint32_t seed = 0;
    int32_t seed_mode = 0;   // uvrt_set_seed_mode

    // knobs
    int32_t sort_bits = 0;   // ray ordering off by default: extend is VALU-bound
    bool record_hits = false;
    int32_t variant = 0;
    int32_t flavour = 0;
    int32_t gather_sampling = 0;   // uvrt_set_gather_sampling: read by uvrt_gather_direct alone
    int32_t gather_variance = 0;   // uvrt_set_gather_variance: uvrt_gather_direct writes the variance plane as well
    int32_t gather_faces = 0;      // uvrt_set_gather_faces: uvrt_gather_direct writes the two face planes as well
#ifdef UVRT_DEV_VARIANTS
    // timing-only probe of the developer build (UVRT_PROBE_SKIP_GENERATE=n): after n uvrt_trace_batch calls the generate
    // launches are skipped -- the buffers still hold the same rays when every computation is the same (bench.py), so
    // the dose stays right and the step shows what k_generate_batch costs the pipeline (an upper bound for any scheme
    // that makes the rays elsewhere)
    int probe_skip_generate = 0;
    int probe_batches = 0;
#endif
    // (a dedupe group's chunks -- gid ranges across its launches, sized by their upper bound of which about half is traced --
    //  pay up to twice the size: profiles/r08/r08_chunk_sweep.txt; the knob sets both)
    size_t dedupe_chunk_bytes = (size_t)192 << 20;
    size_t batch_chunk_bytes = (size_t)96 << 20;   // rays per fused launch of a batch (developer knob UVRT_BATCH_CHUNK_MB,
                                                   // read once in uvrt_create): a chunk's rays stay in the Infinity Cache

    // A deferred accumulate (uvrt_accumulate stores it, its ordering already enqueued on the lane's stream): the Shade that
    // the host loop runs right after a launch (myapp.cpp:159-160) takes it along in ONE kernel (k_accumulate_shade); every
    // other entry point first launches it as the plain k_accumulate (set_device -> flush_pending).  Same arithmetic, same
    // order of operations on the maps: the launch count of an iteration drops from 4 to 3.
    struct PendingAcc { bool valid = false; int lane = 0; float time_step = 0; } pend;
    // traversal error flag + extend timing
    uint32_t* host_flag = nullptr;             // pinned, device-visible host word the kernels raise on a stack overflow: uvrt_sync
    uint32_t* host_flag_dev = nullptr;         // reads it after the stream sync, no copy (its device-side address)
    DevBuf error_flag;                         // (developer build with trip statistics: the flag and the counters behind it)
    hipStream_t probe_stream = nullptr;        // uvrt_clock_probe_start's own stream (created on first use)
    DevBuf probe_out;                          // {shader ticks, 100 MHz ticks}
    bool timing = false;
    std::vector<hipEvent_t> ev_pool;           // start / stop pairs: launch i is timed by events 2 i and 2 i + 1
    size_t ev_used = 0;                        // pairs in use

    // Duration planning (uvrt_plan.hip): exposure matrix, solver buffers; null when no plan is active
    struct PlanState* plan = nullptr;

    // what no member destroys by itself (uvrt_capi.hip): the plan, the hot entries' and the fences' events, the timing
    // pool, the pinned flag, the probe's stream and the context's own
    ~uvrt_ctx();
};

namespace uvrt_impl {
using namespace uvrt;

// ---- launch lanes ----
inline hipStream_t stream_of(uvrt_ctx* c, int l) { return l == 0 ? c->stream : c->lanes[l].side; }
inline Lane& cur_lane(uvrt_ctx* c) { return c->lanes[c->lane]; }
// a side lane's overflow stack: 8 workgroups per CU x 256 threads x 24 entries (the largest grid a side lane runs)
inline size_t side_ovf_bytes(const uvrt_ctx* c) { return (size_t)c->num_cus * 8 * 256 * 24 * sizeof(uint32_t); }

inline int set_device_only(uvrt_ctx* c)
{
    HIP_TRY(hipSetDevice(c->device));
    return UVRT_OK;
}
// the deferred accumulate as a launch of its own, on the stream of the lane it belongs to (ordering enqueued by uvrt_accumulate)
inline int flush_pending(uvrt_ctx* c)
{
    if (!c->pend.valid) return UVRT_OK;
    c->pend.valid = false;
    const int l = c->pend.lane;
    launch_accumulate(c->photon_map.as<double>(), c->max_map.as<double>(), c->lanes[l].counts.as<int32_t>(),
                      c->replicas, c->T, c->pend.time_step, c->T, c->helper_prio, stream_of(c, l));
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}
// every entry point that touches the device starts here (uvrt_shade, which may take a deferred accumulate along, uses
// set_device_only)
inline int set_device(uvrt_ctx* c)
{
    HIP_TRY(hipSetDevice(c->device));
    return flush_pending(c);
}
// the main stream becomes ordered after everything the side streams hold
inline int join_all(uvrt_ctx* c)
{
    for (int l = 1; l < uvrt_ctx::MAXL; ++l) {
        Lane& L = c->lanes[l];
        if (!L.used) continue;
        HIP_TRY(hipEventRecord(L.ev_tail, L.side));
        HIP_TRY(hipStreamWaitEvent(c->stream, L.ev_tail, 0));
        L.used = false;
    }
    return UVRT_OK;
}
// a context-wide operation has been enqueued on the main stream: later side-stream work waits for it
inline int mark_fence(uvrt_ctx* c)
{
    HIP_TRY(hipEventRecord(c->ev_fence, c->stream));
    ++c->fence_seq;
    return UVRT_OK;
}
// an operation on the per-triangle maps (reset, an external reduction) has been enqueued on the main
// stream: later accumulate / Shade work on side streams waits for it -- generate and extend do not,
// so the first launches of the next computation overlap the drain of the previous one
inline int mark_map_fence(uvrt_ctx* c)
{
    HIP_TRY(hipEventRecord(c->ev_mapfence, c->stream));
    ++c->mapfence_seq;
    return UVRT_OK;
}
// stream of the current lane; a side stream first catches up with the last context-wide operation
// and, for work on the maps (`maps`), with the last operation on them
inline int lane_stream(uvrt_ctx* c, hipStream_t* out, bool maps = false)
{
    // external work enqueued on the main stream since a device pointer was handed out
    if (c->ext_touch) { c->ext_touch = false; if (int rc = mark_fence(c)) return rc; }
    if (c->ext_touch_maps) { c->ext_touch_maps = false; if (int rc = mark_map_fence(c)) return rc; }
    if (c->lane == 0) { *out = stream_of(c, 0); return UVRT_OK; }
    Lane& L = cur_lane(c);
    if (c->fence_seq != L.seen_fence) {
        HIP_TRY(hipStreamWaitEvent(L.side, c->ev_fence, 0));
        L.seen_fence = c->fence_seq;
    }
    if (maps && c->mapfence_seq != L.seen_mapfence) {
        HIP_TRY(hipStreamWaitEvent(L.side, c->ev_mapfence, 0));
        L.seen_mapfence = c->mapfence_seq;
    }
    L.used = true;
    *out = L.side;
    return UVRT_OK;
}
// the current lane's stream becomes ordered after everything the previous launch's lane holds (its
// accumulate and Shade): the per-triangle maps are updated in launch order
inline int order_after_previous(uvrt_ctx* c)
{
    const int l = c->lane, q = c->prev_lane;
    if (q == l) return UVRT_OK;
    if (l == 0) return join_all(c);
    HIP_TRY(hipEventRecord(c->lanes[q].ev_tail, stream_of(c, q)));
    HIP_TRY(hipStreamWaitEvent(c->lanes[l].side, c->lanes[q].ev_tail, 0));
    c->lanes[l].used = true;
    return UVRT_OK;
}
// The launch lane of a new per-launch generate: the next one in the rotation when the launch may take part in it
// (`may_pipeline`: what the caller's kind of launch adds to the context's own conditions), else lane 0 behind everything.
inline int next_launch_lane(uvrt_ctx* c, bool may_pipeline)
{
    const bool pipe_ok = may_pipeline && c->pipeline && c->nlanes > 1 && !c->record_hits && c->lanes[1].rays.p;
    c->prev_lane = c->lane;
    c->cur_pipelined = pipe_ok;
    if (pipe_ok) c->lane = (c->lane + 1) % c->nlanes;
    else { if (int rc = join_all(c)) return rc; c->lane = 0; }
    return c->lane == 0 ? UVRT_OK : cur_lane(c).ovf.ensure(side_ovf_bytes(c), false, c->stream);
}
// compute units the persistent grid of a launch on the current lane is sized for
inline int lane_cus(const uvrt_ctx* c) { return c->lane == 0 ? c->num_cus : c->num_cus - c->lanes_masked_cus; }

// bytes between the host and the device over the context's stream, waited for
inline int copy_sync(uvrt_ctx* c, void* dst, const void* src, size_t bytes, hipMemcpyKind kind)
{
    if (bytes == 0) return UVRT_OK;
    HIP_TRY(hipMemcpyAsync(dst, src, bytes, kind, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UVRT_OK;
}
inline bool range_ok(const void* host, int64_t first, int64_t count, int64_t limit)
{
    return host && first >= 0 && count >= 0 && first + count <= limit;
}
// Elements [first, first + count) of a device array of `elem`-byte elements to the host (hipMemcpyDeviceToHost) or from it,
// behind everything the context has outstanding.  The caller has checked the range (range_ok).
inline int range_copy(uvrt_ctx* c, void* base, size_t elem, void* host, int64_t first, int64_t count, hipMemcpyKind kind)
{
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    char* dev = (char*)base + (size_t)first * elem;
    return kind == hipMemcpyDeviceToHost ? copy_sync(c, host, dev, (size_t)count * elem, kind)
                                         : copy_sync(c, dev, host, (size_t)count * elem, kind);
}

// A ray as the ABI hands it over (raytracer.h Ray, 32 bytes) and its split into the device's arrays: {dir, orig.y} per ray
// and, for rays with origins of their own, {orig.x, orig.z} and the distance
struct HostRay { float d[3], o[3], dist; uint32_t tri; };
inline void unpack_rays(const HostRay* hr, int64_t n, std::vector<float>& packed, std::vector<float>* oxz = nullptr,
                        std::vector<float>* tmax = nullptr)
{
    packed.resize((size_t)n * 4);
    if (oxz) oxz->resize((size_t)n * 2);
    if (tmax) tmax->resize((size_t)n);
    for (int64_t i = 0; i < n; ++i) {
        packed[4 * i + 0] = hr[i].d[0]; packed[4 * i + 1] = hr[i].d[1];
        packed[4 * i + 2] = hr[i].d[2]; packed[4 * i + 3] = hr[i].o[1];
        if (oxz) { (*oxz)[2 * i + 0] = hr[i].o[0]; (*oxz)[2 * i + 1] = hr[i].o[2]; }
        if (tmax) (*tmax)[i] = hr[i].dist;
    }
}

// work-item 0's RNG walk of cl/generate.cl:13-39 on the host (strict f32/f64, same order)
inline uint32_t host_wang_hash(uint32_t s)
{
    s = (s ^ 61u) ^ (s >> 16);
    s *= 9u;
    s = s ^ (s >> 4);
    s *= 0x27d4eb2du;
    s = s ^ (s >> 15);
    return s;
}
inline float host_random_float(uint32_t& s)
{
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return (float)s * 2.3283064365387e-10f;
}

inline void split_bits(int bits, int& bphi, int& by, int& bo)
{
    bo = bits / 4;
    bphi = (bits - bo + 1) / 2;
    by = bits - bo - bphi;
}

// Kernel knobs (uvrt_set_variant).  0 (default) = the top-of-tree LDS cache, leaf visits every second
// trip, refill at 8 idle lanes, 8 workgroups per CU; 400-499 = code + 10 * grid code (uvrt_extend6.hip:
// code bits 0-1 leaf period - 1, bit 2 no LDS cache; grid code 0..4 = 8 / 4 / 6 / 2 / 16 workgroups per CU)
// with refill at 16 idle lanes; 500-599 = the same with IEEE divisions everywhere; 600-1299 = like 400-499 with the refill threshold 8 / 24 / 4 / 32 / 40 / 48 / 56 idle
// lanes (hundreds digit 6 ... 12).  (The v1-v5 kernels of round 1 are gone: see git history
// and DESIGN.md section 4 for what they measured.)
#ifdef UVRT_DEV_VARIANTS
inline bool variant_ok(int v) { return v == 0 || (v >= 400 && v < 1300); }
#else      // the product library holds the default kernel only: code 1 (leaf period 2, LDS cache) with any grid / refill knob
inline bool variant_ok(int v) { return v == 0 || (v >= 400 && v < 1300 && v % 10 == 1); }
#endif

inline int auto_sort_bits(int64_t n)
{
    // about one wave (64 rays) per key; no ordering for launches too small to matter
    if (n < 8192) return 0;
    int b = 0;
    while ((int64_t(64) << (b + 1)) <= n && b < 18) ++b;
    return b;
}


inline bool variant_is_knob(int v) { return v >= 400 && v < 1300; }
// idle lanes that trigger a refill.  Default 8; 24 for scenes of a million records and more, where a trip is a miss to the
// fabric whatever its lanes do and fewer, fuller refills are worth 2-3 % (profiles/r03/r03_soup_knobs.txt; the room is flat
// between 8 and 16 and loses at 24)
inline int variant_refill_min(int v, size_t records)
{
    if (!variant_is_knob(v)) return records >= ((size_t)1 << 20) ? 24 : 8;
    return v >= 1200 ? 56 : v >= 1100 ? 48 : v >= 1000 ? 40 : v >= 900 ? 32 : v >= 800 ? 4 : v >= 700 ? 24 : v >= 600 ? 8 : 16;
}
// IEEE divisions for a launch from lamp column (ox, oz): the conditions of the reciprocal shortcut that are uniform over
// the launch (slab<>()), or variants 500-599
inline int variant_force_exact(int v, bool scene_force_exact, float ox, float oz)
{
    const float ax = std::fabs(ox), az = std::fabs(oz);
    const float tiny = 7.888609e-31f;   // 2^-100
    return (scene_force_exact || (ax != 0.0f && ax < tiny) || (az != 0.0f && az < tiny) || !(ax <= 1e9f) || !(az <= 1e9f) ||
            (v >= 500 && v < 600)) ? 1 : 0;
}
inline int variant_code6(int v) { return !variant_is_knob(v) ? 1 : v % 10; }   // default: LDS top cache, leaf period 2
inline int variant_per_cu(int v, int dflt)
{
    static const int per_cu[6] = {8, 4, 6, 2, 16, 7};
    const int gcode = (v / 10) % 10;
    return !variant_is_knob(v) ? dflt : per_cu[gcode < 6 ? gcode : 0];
}
// The record renumbering for a launch from `lamp` on launch lane `lane` (stream `s`): the caller's own
// (uvrt_set_record_perm), the automatic hot-record one (uvrt_hotset.hip: three small kernels enqueued on `s` the
// first time the lamp is seen), or none.  (uvrt_capi_launch.hip)
int launch_perm(uvrt_ctx* c, const float lamp[3], float light_length, uint32_t seed_prev, uint32_t seed_next,
                hipStream_t s, int lane, const uint32_t** out);
// the two halves of launch_perm: the cached renumbering of `lamp` (*out), or a reserved entry (*fresh, its `perm` pointer
// already final) whose set-up hot_build enqueues on `s` -- for several new lamps at once in ONE launch of each kernel
int hot_lookup(uvrt_ctx* c, const float lamp[3], hipStream_t s, const uint32_t** out, uvrt_ctx::HotEntry** fresh);
int hot_build(uvrt_ctx* c, uvrt_ctx::HotEntry* const* entries, const uint32_t* seed_prev, const uint32_t* seed_next, int count,
              float light_length, hipStream_t s, int lane);
// stamp of the renumbering at `perm` (0: none): what a key of prepared records remembers beside the address
inline uint64_t perm_generation(const uvrt_ctx* c, const uint32_t* perm)
{
    if (!perm) return 0;
    if (perm == c->perm.as<uint32_t>()) return c->perm_gen;
    for (const auto& h : c->hot) if (h.perm == perm) return h.gen;
    return 0;
}
// drops every cached renumbering (a new scene); with `slab`, the first slab of the new scene is allocated at once
int hot_reset(uvrt_ctx* c, bool slab);
// waits for the context's stream and deletes the duration-planning state (a new scene, uvrt_plan_end, ~uvrt_ctx)  (uvrt_plan.hip)
void plan_drop(uvrt_ctx* c);
// (re)creates the side lanes' streams with `reserve` CUs masked out, one per XCD and mask word of 8 (0: plain streams)
int set_lane_cu_mask(uvrt_ctx* c, int reserve);
// the scene part of an ExtendParams
inline void fill_scene(const uvrt_ctx* c, ExtendParams& p)
{
    p.scene.pairs = c->pairs.as<PairRec>();
    p.scene.ltris = c->ltris.as<LeafTri>();
    p.scene.leaf_count = c->leaf_count.as<uint32_t>();
    p.scene.root_ref = c->root_ref;
    p.scene.tri_count = c->T;
}
// The launch-uniform part of an ExtendParams for a walk on the current lane from lamp column (ox, oz); the caller adds
// the rays, counts, records, renumbering and (batched) planes
inline void fill_launch(uvrt_ctx* c, ExtendParams& p, float ox, float oz)
{
    memset(&p, 0, sizeof p);
    fill_scene(c, p);
    p.force_exact = variant_force_exact(c->variant, c->scene_force_exact, ox, oz);
    p.error_flag = c->host_flag_dev ? c->host_flag_dev : c->error_flag.as<uint32_t>();
    p.flavour = c->flavour;
    p.top_pairs = c->top_pairs;
    p.ovf_stack = cur_lane(c).ovf.as<uint32_t>();
    p.ovf_capacity = cur_lane(c).ovf.bytes / sizeof(uint32_t);
    p.num_cus = lane_cus(c);
    p.ox = ox;
    p.oz = oz;
    p.npairs = c->npairs;
    p.drain_merge = c->drain_merge;
    p.nearfar_minmax = c->nearfar_minmax;
    p.refill_min = variant_refill_min(c->variant, (size_t)c->npairs + (size_t)c->T);
}
// uvrt_extend for the free rays of the last uvrt_write_free_rays / uvrt_generate_sweep (uvrt_capi_free.hip)
int extend_free(uvrt_ctx* c, int64_t n);
// the scene's free records, made on first use (uvrt_capi_free.hip); make_free_records is its enqueue part for a caller that
// has joined the lanes and marks the fence itself (uvrt_trace_batch)
int ensure_free_records(uvrt_ctx* c);
int make_free_records(uvrt_ctx* c);
// the expected plane of the direct gather, f64[T]: allocated and zeroed on first use (uvrt_capi_gather.hip)
int ensure_expected(uvrt_ctx* c);
// the variance plane beside it, f64[T]: likewise
int ensure_variance(uvrt_ctx* c);
// the direct gather's face planes, f64[2][T]: likewise
int ensure_faces(uvrt_ctx* c);
// the one-bounce gather's source plane, f64[T]: likewise (uvrt_capi_indirect.hip)
int ensure_source(uvrt_ctx* c);
// what the shadow-ray and closest-hit launches share (uvrt_capi_gather.hip): lane 0's ray buffer behind all outstanding work,
// the scene's free records, every ray's {orig.x, orig.z}, tmax and answer byte; the gather's triangles by original id
int begin_shadow_launch(uvrt_ctx* c);
int ensure_gather_tris(uvrt_ctx* c);
// k_occlude_free over the first n rays of lane 0 (rays, g_oxz, g_tmax -> g_occ) on the context's stream; `who` names the call
int trace_shadow_rays(uvrt_ctx* c, int64_t n, const char* who);
// n rays of the ABI (dist = tmax) into lane 0's rays, g_oxz and g_tmax: unpacked, then `begin` (begin_shadow_launch or
// begin_closest_launch), then the three uploads on the context's stream
int upload_query_rays(uvrt_ctx* c, const void* rays32, int64_t n, int (*begin)(uvrt_ctx*));
// The arguments of a query launch (an OccludeParams or a ClosestParams) over the first n rays of lane 0 (rays, g_oxz,
// g_tmax) on the context's stream; the caller adds where the answers go
template <class QueryParams>
inline void fill_query_launch(uvrt_ctx* c, QueryParams& q, int64_t n)
{
    Lane& L = c->lanes[0];
    fill_launch(c, q.e, 0.0f, 0.0f);        // (force_exact: the scene's and the variant's conditions; the origins are per ray)
    q.e.ovf_stack = L.ovf.as<uint32_t>();   // lane 0's, like its rays: this launch runs on the context's stream
    q.e.ovf_capacity = L.ovf.bytes / sizeof(uint32_t);
    q.e.num_cus = c->num_cus;
    q.e.rays = L.rays.as<float4>();
    q.oxz = c->g_oxz.as<float2>();
    q.tmax = c->g_tmax.as<float>();
    q.e.n = n;
    q.e.recs = c->derived.free_recs.p;
}
// A gather's triangles in chunks of floor(capacity / S): a triangle's S samples never straddle two of them, so the chunking
// shows in no bit.  each(done, cnt) works on the cnt triangles behind the first `done` and returns a status; the first that
// is not UVRT_OK ends the walk and is returned.
inline int32_t tris_per_chunk(const uvrt_ctx* c, int32_t S) { return (int32_t)std::min<int64_t>(c->capacity / S, INT32_MAX); }
template <class Each>
inline int for_tri_chunks(const uvrt_ctx* c, int32_t S, int32_t tri_count, Each&& each)
{
    const int32_t per_chunk = tris_per_chunk(c, S);
    for (int32_t done = 0; done < tri_count; done += per_chunk)
        if (int rc = each(done, std::min(per_chunk, tri_count - done))) return rc;
    return UVRT_OK;
}
// what the one-bounce gather and the link build share (uvrt_capi_indirect.hip): begin_shadow_launch plus the hit records;
// the argument check (`who` names the call in the message); the generate kernel's arguments; k_closest_free over the first
// n rays of lane 0 (rays, g_oxz, g_tmax -> g_hit) on the context's stream
int begin_closest_launch(uvrt_ctx* c);
int check_indirect(uvrt_ctx* c, const uvrt_indirect_params* prm, int32_t first_tri, int32_t tri_count, const char* who);
IndirectGenParams indirect_gen_params(uvrt_ctx* c, const uvrt_indirect_params* prm);
int trace_closest_rays(uvrt_ctx* c, int64_t n, const char* who);
// the next pair of the extend timing pool (uvrt_extend_time_ms) with its start recorded on `s`; *stop stays null
// while timing is off
inline int timing_start(uvrt_ctx* c, hipStream_t s, hipEvent_t* stop)
{
    *stop = nullptr;
    if (!c->timing) return UVRT_OK;
    while (c->ev_pool.size() < 2 * (c->ev_used + 1)) {      // (the pool owns an event from the moment it exists)
        hipEvent_t e;
        HIP_TRY(hipEventCreate(&e));
        c->ev_pool.push_back(e);
    }
    const size_t i = c->ev_used++;
    HIP_TRY(hipEventRecord(c->ev_pool[2 * i], s));
    *stop = c->ev_pool[2 * i + 1];
    return UVRT_OK;
}
// A traversal launch on `s` between the events of a timing pair.  `launch` enqueues it and returns false when its grid needs
// more overflow-stack entries than the lane's buffer holds; `what` names the launch in that error.
template <class Launch>
inline int timed_launch(uvrt_ctx* c, hipStream_t s, const char* who, const char* what, Launch&& launch)
{
    hipEvent_t stop;
    if (int rc = timing_start(c, s, &stop)) return rc;
    if (!launch())
        return fail(UVRT_ERR_INVALID, "%s: %s with variant %d needs a larger overflow-stack buffer than the context holds", who,
                    what, c->variant);
    HIP_TRY(hipGetLastError());
    if (stop) HIP_TRY(hipEventRecord(stop, s));
    return UVRT_OK;
}

}  // namespace uvrt_impl

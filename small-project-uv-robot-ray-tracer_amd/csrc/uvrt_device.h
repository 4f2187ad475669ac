// uvrt_device.h -- device-side record layouts and kernel launch wrappers (gfx950 only).
//
// HBM layout of one context (see DESIGN.md "Data layout"):
//   pairs    : one 64-byte record per INNER node = the AABBs of its two children plus a 32-bit
//              reference to each child.  The reference's traversal always touches the two
//              children of a node together (extend.cl:56-59), so one aligned 64-byte record
//              (4 x dwordx4) replaces two 32-byte BVHNode gathers.
//   ltris    : one 48-byte record per triIdx slot (leaf order): v0, e1 = v1-v0, e2 = v2-v0 and
//              the original triangle id.  Replaces the triIdx[] -> Triangle[] double
//              indirection of extend.cl:50-53.
//   rays     : 16 bytes per photon {dir.xyz, orig.y}; orig.x / orig.z are the lamp's and are
//              launch-uniform (generate.cl:16).
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>
#include "uvrt_dedupe.h"

namespace uvrt {

constexpr uint32_t REF_LEAF_BIT = 0x80000000u;   // bit 31: leaf reference
constexpr uint32_t REF_DONE = 0xFFFFFFFFu;       // traversal finished
constexpr uint32_t REF_FIRST_MASK = 0x07FFFFFFu; // leaf: first slot in ltris (27 bits)
constexpr int REF_COUNT_SHIFT = 27;              // leaf: 4-bit count code, 15 = see leaf_count[]
constexpr int MAX_TRIS = 1 << 27;

struct alignas(16) PairRec {   // 64 B
    float4 c0min_ref0;         // child0 min.xyz, bits of ref0
    float4 c0max_ref1;         // child0 max.xyz, bits of ref1
    float4 c1min;              // child1 min.xyz, 0
    float4 c1max;              // child1 max.xyz, 0
};

struct alignas(16) LeafTri {   // 48 B
    float4 v0_id;              // v0.xyz, bits of the original triangle id
    float4 e1;                 // v1 - v0 (one f32 subtraction per component, extend.cl:13)
    float4 e2;                 // v2 - v0
};

// 4-wide node of the opt-in collapsed tree (uvrt_extend4.hip): the boxes of up to four children -- the
// grandchildren of a node of the reference's BVH2 where its children are inner nodes -- and a reference to
// each.  128 bytes = two 64-byte record units; an empty slot holds a box no ray can hit and REF_DONE.
struct alignas(16) QuadRec {
    float4 xz[4];              // child k: min.x, max.x, min.z, max.z  (per launch: minus the lamp's x / z)
    float4 y01, y23;           // c0 min.y, c0 max.y, c1 min.y, c1 max.y ; likewise c2, c3
    uint32_t ref[4];           // inner: unit index (2 x node index); leaf: as in the BVH2 form, re-based per launch
    uint32_t pad[4];
};

struct SceneDev {
    const PairRec* pairs;
    const LeafTri* ltris;
    const uint32_t* leaf_count;  // per ltris slot: triangle count of the leaf starting there
    uint32_t root_ref;
    int32_t tri_count;
};

// One per-launch node-pair record of extend v6 (layout: uvrt_extend6.hip): the lamp's x / z
// subtracted from the x / z bounds (the single f32 subtraction of extend.cl:31,35), one axis of one
// child per register pair, leaf references re-based to record indices.
// `perm` (or nullptr = identity) renumbers the pair records: record i is written at perm[i] and the
// inner references are translated, so that the records the lamp's rays visit most form the prefix
// that the kernel serves from LDS.
__device__ __forceinline__ void ascending(float& lo, float& hi)
{
    if (hi < lo) { const float t = lo; lo = hi; hi = t; }
}
__device__ __forceinline__ void prepare_record6(const PairRec* __restrict__ pairs, float4* __restrict__ recs,
                                                float ox, float oz, int32_t npairs, int src,
                                                const uint32_t* __restrict__ perm)
{
    const PairRec pr = pairs[src];
    uint32_t r0 = __float_as_uint(pr.c0min_ref0.w), r1 = __float_as_uint(pr.c0max_ref1.w);
    if (r0 >= REF_LEAF_BIT) r0 += (uint32_t)npairs; else if (perm) r0 = perm[r0];
    if (r1 >= REF_LEAF_BIT) r1 += (uint32_t)npairs; else if (perm) r1 = perm[r1];
    const int i = perm ? (int)perm[src] : src;
    float4 w0 = make_float4(pr.c0min_ref0.x - ox, pr.c0max_ref1.x - ox, pr.c0min_ref0.z - oz, pr.c0max_ref1.z - oz);
    float4 w1 = make_float4(pr.c1min.x - ox, pr.c1max.x - ox, pr.c1min.z - oz, pr.c1max.z - oz);
    float4 w2 = make_float4(pr.c0min_ref0.y, pr.c0max_ref1.y, pr.c1min.y, pr.c1max.y);
    // every pair in ascending order: k_extend6's stream takes the nearer slab distance of a pair from the sign of the ray's
    // direction alone.  A no-op for a box with min <= max; an inverted box keeps both values (every other consumer takes the
    // min and the max of the pair's two distances); a pair with a NaN stays as it is.
    ascending(w0.x, w0.y); ascending(w0.z, w0.w);
    ascending(w1.x, w1.y); ascending(w1.z, w1.w);
    ascending(w2.x, w2.y); ascending(w2.z, w2.w);
    recs[i * 4 + 0] = w0;
    recs[i * 4 + 1] = w1;
    recs[i * 4 + 2] = w2;
    recs[i * 4 + 3] = make_float4(__uint_as_float(r0), __uint_as_float(r1), 0.f, 0.f);
}

// ---- instruction-issue priority of the short kernels (include/uvrt.h uvrt_set_helper_priority) ----
// Issue on a SIMD is arbitrated by priority, then age.  A short kernel that runs beside the other lane's persistent traversal
// grid is the youngest wave on its SIMD, next to seven issue-bound traversal waves at priority 0, and gets the slots they
// leave.  Called first in such a kernel with the context's setting (a kernel argument, so wave-uniform: s_setprio ignores
// EXEC and must sit behind a scalar branch), it lets the wave issue when it is ready.  0 leaves the wave as it starts.
__device__ __forceinline__ void helper_priority(int prio)
{
    switch (prio) {
        case 1: __builtin_amdgcn_s_setprio(1); break;
        case 2: __builtin_amdgcn_s_setprio(2); break;
        case 3: __builtin_amdgcn_s_setprio(3); break;
        default: break;
    }
}

// ------------------------------------------------------------------ RNG, cl/tools.cl:2-4

__device__ __forceinline__ uint32_t wang_hash(uint32_t s)
{
    s = (s ^ 61u) ^ (s >> 16);
    s *= 9u;
    s = s ^ (s >> 4);
    s *= 0x27d4eb2du;
    s = s ^ (s >> 15);
    return s;
}

__device__ __forceinline__ float random_float(uint32_t& s)
{
    s ^= s << 13;
    s ^= s >> 17;
    s ^= s << 5;
    return (float)s * 2.3283064365387e-10f;
}

// cl/generate.cl:11-37 for work-item `gid`: returns {dir.xyz, orig.y} (orig.x / orig.z are the lamp's).
// r0 = the first random float (position on the rod), (x, y) = the accepted disc sample: for the optional
// coherence key of k_generate.  seed_mode: include/uvrt.h uvrt_set_seed_mode.
// `seed` returns the work-item's RNG state after its last draw (what a sweep goes on drawing from, uvrt_extend_free.hip).
__device__ __forceinline__ float4 generate_ray_rng(float lx, float ly, float lz, float light_length, int64_t gid,
                                                   uint32_t seed_prev, uint32_t seed_next, int32_t seed_mode,
                                                   float& r0, double& x, double& y, uint32_t& seed)
{
    seed = wang_hash(seed_input(gid, lx, ly, lz, seed_prev, seed_next, seed_mode));      // generate.cl:11-13 (uvrt_dedupe.h)

    r0 = random_float(seed);
    const float origy = ly + r0 * light_length;          // :16
    const float diry = random_float(seed) * 2.0f - 1.0f; // :22
    const double dirxzlength = sqrt(1.0 - (double)diry * (double)diry);   // :23

    x = (double)(random_float(seed) * 2.0f - 1.0f);                       // :25
    y = (double)(random_float(seed) * 2.0f - 1.0f);
    while (x * x + y * y > 1.0) {                                         // :26-28
        x = (double)(random_float(seed) * 2.0f - 1.0f);
        y = (double)(random_float(seed) * 2.0f - 1.0f);
    }
    const double s = dirxzlength / sqrt(x * x + y * y);                   // :29
    return make_float4((float)(x * s), diry, (float)(y * s), origy);      // :31-37
}
__device__ __forceinline__ float4 generate_ray(float lx, float ly, float lz, float light_length, int64_t gid,
                                               uint32_t seed_prev, uint32_t seed_next, int32_t seed_mode,
                                               float& r0, double& x, double& y)
{
    uint32_t seed;
    return generate_ray_rng(lx, ly, lz, light_length, gid, seed_prev, seed_next, seed_mode, r0, x, y, seed);
}

// ---- the traversal kernel's LDS cache (uvrt_extend6.hip) ----
constexpr uint32_t TOP6_MAX = 175;        // records cached in LDS: 176 x 64 B + 9 stack rows = 20 KB per workgroup, eight per CU

// ---- batched tracing (include/uvrt.h uvrt_trace_batch): several launches' rays side by side ----
// (MAX_BATCH, the launches per uvrt_trace_batch / uvrt_replay_batch call, and MAX_CLASS_PLANES: uvrt_dedupe.h)
struct GenBatchParams {
    float4* rays;                      // [count][n_pad]: physical plane p at rays + p * n_pad
    int64_t n_pad;                     // rays per plane in the buffer (n rounded up to 64)
    int64_t first_gid, n;              // global ids [first_gid, first_gid + n) of EVERY launch
    float light_length;
    int32_t seed_mode;
    int32_t count;
    float lx[MAX_BATCH], ly[MAX_BATCH], lz[MAX_BATCH];       // lamp of physical plane p
    uint32_t seed_prev[MAX_BATCH], seed_next[MAX_BATCH];     // its place in the SEED chain
    int32_t prio;                      // helper_priority
};

// The distinct rays of a dedupe group (uvrt_dedupe.h) over the gids [g0, g0 + gn) of all its launches, compacted: the owners'
// rays in (launch, gid) order with their masks beside them.  Three kernels: mark (the owner test over strips of key tiles, a count per
// launch and block of DD_SLOTS gids), scan, write (the f64 direction code, for owners only).  The order is a function of the
// group alone; the count stays on the device.
constexpr int DD_ROUNDS = 8, DD_SLOTS = 256 * DD_ROUNDS;      // gids per workgroup of the write pass and per owner count
struct GenDedupeParams {
    DedupeGroup g;
    float4* rays;                      // out: [*total] <= count * gn
    uint32_t* masks;                   // out: parallel to rays, each ray's deposit word (uvrt_dedupe.h "mask classes")
    uint32_t* total;                   // out: rays written
    uint32_t* tmp;                     // scratch [count][gn]: every occurrence's mask between the passes
    uint32_t* block_counts;            // scratch [count * ceil(gn / 2048)] (sized for ceil(gn / 256) by the caller): ZERO before
                                       // mark, which adds the owners; offsets after the scan; write leaves it zero again
    int64_t g0, gn;
    int64_t key_lo, tiles;             // the chunk's key tiles (dedupe_tile_range with DEDUPE_MARK_KEYS)
    int32_t strip_tiles;               // consecutive tiles a wave of the mark pass walks (at least 1)
    float light_length;
    int32_t prio;                      // helper_priority of the three kernels
    uint32_t* deposits;                // out: the atomics these rays issue when each of them hits (dedupe_word_deposits summed)
    DedupeClasses cls;                 // the group's mask classes (count 0: masks[] holds the masks themselves)
    // the period table (uvrt_dedupe.h "period table"): mark walks the key intervals between the interiors (gaps >= 1; without a
    // table one gap, the chunk's key tiles) and counts the interiors' owners from the table, write reads their words from it
    DedupePeriodic per;
    int32_t gaps;
    int32_t gap_key[DEDUPE_PERIODIC_STRATA + 1];
    uint32_t gap_keys[DEDUPE_PERIODIC_STRATA + 1];
    int32_t gap_strip0[DEDUPE_PERIODIC_STRATA + 2];      // gap i: the workgroups [gap_strip0[i], gap_strip0[i + 1]) of the mark pass
};
static_assert(sizeof(GenDedupeParams) <= 3584, "kernel arguments: 4 KB with the hidden ones");
void launch_generate_dedupe(const GenDedupeParams& p, hipStream_t s);
// its first kernel alone: tmp and the owners per block added to block_counts (a test hook runs it by itself)
void launch_dedupe_mark(const GenDedupeParams& p, hipStream_t s);
// k_extend6 over such a list (p.masks, p.n_dev, p.n = the upper bound, p.plane_stride = ints between planes)
struct ExtendParams;
bool launch_extend6_dedupe(const ExtendParams& p, int code, int grid_per_cu, hipStream_t s);

// one entry of uvrt_replay_batch, in LOGICAL launch order
struct ReplayOp {
    int32_t plane;                     // physical plane of this launch
    float duration;                    // accumulate.cl timeStep
    int32_t shade;                     // run computeDosage + dosageToColor after this launch
    int32_t which_map;                 // 0 photonMap, 1 maxPhotonMap
    int32_t photons_per_light;
    float scaled_power, min_value;
    int32_t threshold_view;
};

struct ReplayParams {
    double* photon_map;
    double* max_map;
    int32_t* planes;                   // [plane][replicas][T] deposit replicas (folded == 0)
    int32_t* folded;                   // [plane][T] sums over the replicas (folded == 1)
    float* dosage;
    float* color;
    const float* area;
    int64_t plane_stride;              // ints between planes of `planes` (= replicas * T)
    int32_t replicas, T, count, is_folded;      // T: the scene's triangles, the stride of a replica and of a folded plane
    int32_t prio;                      // helper_priority
    int32_t bound;                     // triangles [0, bound) are replayed (uvrt_replay_batch's tri_count <= T)
    // the mask classes of the batch's dedupe groups (uvrt_dedupe.h): class plane c is plane `nplanes + c` of `planes`, with
    // cls_replicas replicas in use; class_of[k] = the class planes whose mask holds logical launch k
    int32_t nplanes, ncls, cls_replicas;
    uint64_t class_of[MAX_BATCH];
    ReplayOp ops[MAX_BATCH];
};

// the class planes of a batch added into the folded planes of the launches their masks hold, and zeroed
struct FoldClassParams {
    int32_t* planes;                   // the batch set's planes: class plane c at planes + (nplanes + c) * plane_stride
    int32_t* folded;                   // [nplanes][T], after launch_fold_planes
    int64_t plane_stride;
    int32_t nplanes, ncls, cls_replicas, T, prio;
    uint64_t launches[MAX_CLASS_PLANES];     // physical planes class c is added to
};
void launch_fold_classes(const FoldClassParams& p, hipStream_t s);

struct GenParams {
    float4* rays;          // [n] gid order: dir.xyz, orig.y
    uint2* keyrank;        // [n] (key, rank within key) or nullptr when not sorting
    uint32_t* hist;        // [1 << sort_bits]
    float lx, ly, lz;      // lamp position (generate.cl arg 1)
    float light_length;    // generate.cl arg 2
    int64_t first_gid;
    int64_t n;
    uint32_t seed_prev;    // SEED_{k-1}: read by work-item 0
    uint32_t seed_next;    // SEED_k: read by everybody else
    int32_t seed_mode;     // 0 canonical (above); 1 "gfx950-ocl": every work-item reads SEED_{k-1} and a
                           // negative seed sum converts to 0 (include/uvrt.h uvrt_set_seed_mode)
    int32_t bits_phi, bits_y, bits_o;
    // extend v6's per-launch records, written by extra workgroups of the same launch (or nullptr)
    const PairRec* prep_pairs;
    float4* prep_recs;
    const uint32_t* prep_perm;
    int32_t prep_npairs;
    uint32_t ray_blocks;   // workgroups [0, ray_blocks) generate rays, the rest prepare records
    int32_t prio;          // helper_priority
};

struct ExtendParams {
    SceneDev scene;
    const float4* rays;      // [n] in trace order
    uint32_t chunk;          // persistent kernel: trace slots owned by each wavefront
    int32_t cls_replicas;    // a deduped chunk whose `masks` (below) are deposit words (uvrt_dedupe.h "mask classes"; 0: they are the masks themselves): a class plane takes
                             // deposits in its first cls_replicas replicas only -- a class holds a fraction of a launch's rays, and
                             // the replay reads every replica in use.  (It sits in the padding before the next pointer: no other
                             // field moves, and the kernels that do not read it keep their code.)
    uint32_t* ovf_stack;     // persistent kernels: [grid threads][MAX_STACK - LDS entries] stack overflow
    uint64_t ovf_capacity;   // entries (uint32) available in ovf_stack; launches that need more are refused
    int32_t num_cus;         // compute units of the device (persistent grids are sized from it)
    uint32_t top_pairs;      // pair records [0, top_pairs) = the tree levels cached in LDS (<= TOP6_MAX)
    int32_t force_exact;     // scene or lamp position outside the fast path's proof conditions
    int32_t drain_merge;     // k_extend6: the four waves of a workgroup pool the last rays of their drains in one wave (merge6)
    int32_t nearfar_minmax;  // k_extend6, developer build: the stream's min/max near / far block instead of the sign-ordered one
    int32_t flavour;         // 0 strict (canonical), 1 "ocl-amd" fused cross/dot in the triangle test
    const uint32_t* order;   // [n] trace slot -> local ray index, or nullptr (identity)
    uint2* hits;             // [n] by local ray index: (dist bits, triID), or nullptr
    int32_t* counts;         // tempPhotonMap, count_replicas copies count_stride ints apart: a
                             // workgroup deposits into copy (blockIdx % count_replicas), so hits on
                             // a hot triangle do not serialise on one address; accumulate folds them
    int32_t count_replicas;
    int64_t count_stride;
    uint32_t* error_flag;    // set to 1 on traversal stack overflow
    float ox, oz;            // launch-uniform origin components
    int64_t n;
    int32_t npairs;
    void* recs;              // extend v6: [npairs] per-launch pair records + [T] leaf records, 64 B each
    int32_t refill_min;      // extend v6: idle lanes that trigger a refill (16)
    const uint32_t* perm;    // extend v6: record renumbering (nullptr = identity), see prepare_record6
    int32_t recs_prepared;   // extend v6: recs[0, npairs) already hold this launch's records (k_generate)
    uint32_t root_ref6;      // root reference in v6's record numbering (set by launch_extend6)
    // batched tracing: `rays` holds nplanes planes of plane_batches * 64 slots each, of which the first
    // plane_n are rays; the deposits of plane k go to counts + k * plane_stride (+ replica * count_stride).
    // plane_batches == 0: one launch, n rays, no planes.
    uint32_t plane_batches;
    uint32_t plane_n;
    uint32_t plane_stride;
    float plane_inv;         // 1 / plane_batches (set by the launch wrapper): first guess of a batch's plane
    // the 4-wide form (uvrt_extend4.hip): per-launch records [2 * nquads units of 64 B] + leaf records
    const void* recs4;
    int32_t nquads;
    uint32_t top_quads;      // nodes [0, top_quads) are served from LDS
    uint32_t root_ref4;      // REF_DONE / a leaf reference (re-based) / 0
    // a deduped chunk of a batch (launch_extend6_dedupe; uvrt_dedupe.h): `rays` is a compacted list of *n_dev distinct rays
    // (n is its upper bound: the grid is sized from it), masks[i] = the planes ray i deposits in, bit k = plane k of `counts`
    // -- or, where cls_replicas != 0, its deposit word (uvrt_dedupe.h "mask classes")
    const uint32_t* masks;
    const uint32_t* n_dev;
};

// launch wrappers (uvrt_kernels.hip).  `prio` (a params struct's field, or the argument before the stream) is the
// helper_priority of the kernels that can run beside a traversal grid: the caller passes the context's helper_prio.
void launch_generate(const GenParams& p, hipStream_t s);
void launch_generate_batch(const GenBatchParams& p, hipStream_t s);
// folded[p][i] = sum over the replicas of plane p, replicas zeroed (the all-reduce payload)
void launch_fold_planes(int32_t* planes, int32_t* folded, int32_t nplanes, int32_t replicas, int32_t T, int prio, hipStream_t s);
void launch_replay_batch(const ReplayParams& p, hipStream_t s);
void launch_add_counts(int32_t* dst, const int32_t* src, int64_t n, hipStream_t s);     // dst[i] += src[i]
void launch_prepare_launch6(const PairRec* pairs, void* recs, float ox, float oz, int32_t npairs, const uint32_t* perm,
                            int prio, hipStream_t s);
void launch_scan_bins(uint32_t* hist, uint32_t* bin_start, int32_t nbins, hipStream_t s);
void launch_scatter(const float4* rays, const uint2* keyrank, const uint32_t* bin_start,
                    float4* sorted, uint32_t* order, int64_t n, hipStream_t s);
// extend (uvrt_extend6.hip): code bits 0-1 = leaf period - 1, bit 2 = no LDS top cache; returns false
// (nothing launched) when the grid would not fit the overflow-stack buffer.  prep_prio: the helper_priority of the
// k_prepare_launch6 it runs first where the records are not prepared (the traversal itself takes none)
bool launch_extend6(const ExtendParams& p, int code, int grid_per_cu, int prep_prio, hipStream_t s);
// the opt-in 4-wide traversal (uvrt_extend4.hip)
bool launch_extend4(const ExtendParams& p, int grid_per_cu, hipStream_t s);
void launch_prepare_launch4(const QuadRec* quads, void* recs4, float ox, float oz, int32_t nquads, hipStream_t s);
// hot-record set-up (uvrt_hotset.hip): visit statistics -> selection -> renumbering for up to HS_GROUPS lamps at once
constexpr int HS_GROUPS = 16;
struct HotSetupParams {
    const PairRec* pairs;
    const LeafTri* ltris;
    const uint32_t* leaf_count;
    uint32_t root_ref;
    float light_length;
    int32_t seed_mode;
    int32_t n;                         // photons of the launch whose visits are counted (global ids [0, n))
    int32_t npairs, keep, count;       // records, hot records wanted, lamps
    int32_t tail_lanes;                // a wave of k_visit_stats stops once at most this many of its rays are under way
    int32_t direct_bins;               // k_select_hot looks for the hot records among the first direct_bins records before it walks the tree
    uint32_t* hist;                    // [count][npairs] visit counters: zero before, zero again after
    uint32_t* hot_list;                // [count][TOP6_MAX + 1] scratch: number of hot records + their indices, ascending
    uint32_t* perm[HS_GROUPS];         // out: the renumbering of lamp k, [npairs]
    float lx[HS_GROUPS], ly[HS_GROUPS], lz[HS_GROUPS];
    uint32_t seed_prev[HS_GROUPS], seed_next[HS_GROUPS];
};
void launch_hot_setup(const HotSetupParams& p, hipStream_t s);
void launch_prepare_leaves6(const LeafTri* ltris, void* recs, int32_t npairs, int32_t T, hipStream_t s);
constexpr uint64_t OVF_MAX_ENTRIES = (uint64_t)256 * 16 * 256 * 24;   // largest grid x deepest overflow
void launch_accumulate(double* photon_map, double* max_map, int32_t* counts, int32_t replicas,
                       int64_t stride, float time_step, int32_t T, int prio, hipStream_t s);
void launch_reset(double* photon_map, double* max_map, int32_t* counts, int32_t replicas,
                  int64_t stride, float* color, int32_t reset_color, int32_t T, int prio, hipStream_t s);
void launch_fold_counts(int32_t* counts, int32_t replicas, int64_t stride, int32_t T, hipStream_t s);
void launch_compute_dosage(const double* map, float* dosage, const float* area,
                           int32_t photons_per_light, float scaled_power, int32_t T,
                           hipStream_t s);
void launch_shade(const double* map, float* dosage, const float* area, float* color, int32_t photons_per_light,
                  float scaled_power, float min_value, int32_t threshold_view, int32_t T, int prio, hipStream_t s);
void launch_accumulate_shade(double* photon_map, double* max_map, int32_t* counts, int32_t replicas, int64_t stride,
                             float time_step, float* dosage, const float* area, float* color, int32_t which_map,
                             int32_t photons_per_light, float scaled_power, float min_value, int32_t threshold_view,
                             int32_t T, int prio, hipStream_t s);
void launch_dosage_to_color(const float* dosage, float* color, float min_value,
                            int32_t threshold_view, int32_t T, hipStream_t s);
void launch_prepare_scene(const float4* tris64, const uint32_t* tri_idx, LeafTri* ltris,
                          float* area, int32_t T, hipStream_t s);
void launch_clock_probe(unsigned long long* out2, unsigned long long ticks_100mhz, hipStream_t s);
void launch_export_rays(const float4* rays, const uint2* hits, void* out32, float ox, float oz,
                        int64_t first, int64_t count, hipStream_t s);

// ---- rays with origins of their own (uvrt_extend_free.hip) ----
// The free-origin traversal's arguments: an ExtendParams as launch_extend6 takes it (rays = the 16-byte {dir.xyz, orig.y}
// records, recs = the scene's free records, ox / oz unused) plus the rays' {orig.x, orig.z}.
struct FreeParams {
    ExtendParams e;
    const float2* oxz;       // [n] in gid order; batched (launch_extend_free_planes): [plane][n_pad], indexed like e.rays
};
// a lamp that moves from `from` to `to` (include/uvrt.h uvrt_generate_sweep)
struct SweepParams {
    float4* rays;            // [n] dir.xyz, orig.y
    float2* oxz;             // [n] orig.x, orig.z
    float fx, fy, fz, tx, ty, tz;
    float light_length;
    int64_t first_gid, n;
    uint32_t seed_prev, seed_next;
    int32_t prio;            // helper_priority
};
// The scene's free records, made once per scene: pair record i in the layout of prepare_record6 with the RAW bounds (a
// ray subtracts its own origin) in breadth-first order, leaf references re-based; the leaf records follow at [npairs, npairs + T).
void launch_prepare_free_records(const PairRec* pairs, const LeafTri* ltris, void* recs, int32_t npairs, int32_t T, hipStream_t s);
// workgroups per CU the free kernel is resident with (its register allocation decides)
constexpr int FREE_GRID_PER_CU = 8;
bool launch_extend_free(const FreeParams& p, int grid_per_cu, hipStream_t s);
void launch_generate_sweep(const SweepParams& p, hipStream_t s);
// batched tracing (include/uvrt.h uvrt_trace_batch_launches): the rays of up to MAX_BATCH sweeps side by side, as
// GenBatchParams holds those of stops
struct SweepBatchParams {
    float4* rays;                      // [count][n_pad]
    float2* oxz;                       // [count][n_pad]
    int64_t n_pad;
    int64_t first_gid, n;              // global ids [first_gid, first_gid + n) of EVERY sweep
    float light_length;
    int32_t count;
    float fx[MAX_BATCH], fy[MAX_BATCH], fz[MAX_BATCH];       // `from` of physical plane p
    float tx[MAX_BATCH], ty[MAX_BATCH], tz[MAX_BATCH];       // `to`
    uint32_t seed_prev[MAX_BATCH], seed_next[MAX_BATCH];     // its place in the SEED chain
    int32_t prio;                      // helper_priority
};
void launch_generate_sweep_batch(const SweepBatchParams& p, hipStream_t s);
// the free-origin traversal over the planes of a batch: e.plane_batches / plane_n / plane_stride as launch_extend6 takes
// them, every plane's deposits in its own count plane.  No hit records (a batch never records hits).
bool launch_extend_free_planes(const FreeParams& p, int grid_per_cu, hipStream_t s);
void launch_export_free_rays(const float4* rays, const float2* oxz, const uint2* hits, void* out32, int64_t first,
                             int64_t count, hipStream_t s);

// ---- shadow rays and the direct gather (uvrt_occlude.hip; include/uvrt.h "shadow rays and the direct gather") ----
// The occlusion traversal's arguments: a FreeParams (counts, hits and planes unused) plus every ray's tmax and the byte it
// answers with: occluded[i] = some triangle is hit with 0.0001f < t < tmax[i].
struct OccludeParams {
    ExtendParams e;
    const float2* oxz;       // [n] orig.x, orig.z
    const float* tmax;       // [n]
    uint8_t* occluded;       // [n]
};
bool launch_occlude_free(const OccludeParams& p, int grid_per_cu, hipStream_t s);
// n = cross(e1, e2) in f64 and its length: the one expression of the gather, refine, bounce and link kernels (each is built
// without contraction, every operator is one rounding)
__device__ __forceinline__ double tri_normal(const float4 e1, const float4 e2, double& nx, double& ny, double& nz)
{
    const double ax = (double)e1.x, ay = (double)e1.y, az = (double)e1.z;
    const double bx = (double)e2.x, by = (double)e2.y, bz = (double)e2.z;
    nx = ay * bz - az * by;
    ny = az * bx - ax * bz;
    nz = ax * by - ay * bx;
    return sqrt(nx * nx + ny * ny + nz * nz);
}
// the triangles by ORIGINAL id, 3 x float4 each: v0, e1 = v1 - v0, e2 = v2 - v0 (the leaf records' own values, scattered by
// their id; a triangle no leaf holds stays zero: no area, no estimate)
void launch_gather_tris(const LeafTri* ltris, float4* gtris, int32_t T, hipStream_t s);
struct GatherGenParams {
    const float4* gtris;
    float4* rays;            // [tri_count * samples] dir.xyz, orig.y
    float2* oxz;             // orig.x, orig.z
    float* tmax;
    double* w;               // the sample's weight (0 for a sample that is not traced)
    float fx, fy, fz, tx, ty, tz;
    float light_length;
    uint32_t seed_hash;      // WangHash(seed)
    int32_t first_tri, tri_count, samples;
    uint32_t seed;           // the raw seed: the stratified rule hashes it again for the triangle's rotation
    int32_t mode;            // UVRT_GATHER_INDEPENDENT / UVRT_GATHER_STRATIFIED: which instantiation is launched
};
void launch_gather_generate(const GatherGenParams& p, hipStream_t s);
void launch_gather_reduce(const float4* gtris, const double* w, const uint8_t* occluded, double* expected, int32_t first_tri,
                          int32_t tri_count, int32_t samples, int32_t photons_equiv, hipStream_t s);
// the same reduction with variance[t], the estimate's variance, beside expected[t] (the same bits): `mode` picks the sample
// variance of the mean (independent samples) or successive differences (stratified); samples >= 2
void launch_gather_reduce_var(const float4* gtris, const double* w, const uint8_t* occluded, double* expected, double* variance,
                              int32_t first_tri, int32_t tri_count, int32_t samples, int32_t photons_equiv, int32_t mode,
                              hipStream_t s);
// the face-resolved gather (include/uvrt.h "face-resolved gather and bounces"): launch_gather_generate that also writes
// face[i], the face sample i arrives on, and the reduction of the chunk into faces[f * T + t], f64[2][T], beside the reduce above
void launch_gather_generate_faces(const GatherGenParams& p, uint8_t* face, hipStream_t s);
void launch_gather_reduce_faces(const float4* gtris, const double* w, const uint8_t* occluded, const uint8_t* face, double* faces,
                                int32_t first_tri, int32_t tri_count, int32_t samples, int32_t photons_equiv, int32_t T, hipStream_t s);
// accumulate.cl:4-14 with expected[t] in place of (double)tempPhotonMap[t]; the plane is zeroed like tempPhotonMap
void launch_accumulate_expected(double* photon_map, double* max_map, double* expected, float time_step, int32_t T, hipStream_t s);

// ---- the batched direct gather (uvrt_gather_batch.hip; include/uvrt.h "batched direct gather") ----
// One launch of a batch as the kernels read it from the device table: 48 bytes, so three 16-byte loads.
struct alignas(16) GatherBatchLaunch {
    float fx, fy, fz, tx, ty, tz;
    float light_length;
    uint32_t seed;           // the raw seed
    uint32_t seed_hash;      // WangHash(seed)
    int32_t photons_equiv;
    int32_t pad[2];
};
// A chunk of a batch: pairs [first_pair, first_pair + pair_count) of the launch-major sequence q = k * tri_count + lt, given as
// k0 = first_pair / tri_count and lt0 = first_pair % tri_count (host, int64).  Pair p of the chunk is launch
// k0 + (lt0 + p) / tri_count, triangle first_tri + (lt0 + p) % tri_count; its samples are rays [p * samples, (p + 1) * samples)
// of the chunk.  pair_count * samples <= capacity, and lt0 + p < 2^32.
struct GatherBatchParams {
    const float4* gtris;
    const GatherBatchLaunch* table;    // [count]
    float4* rays;            // [pair_count * samples] dir.xyz, orig.y
    float2* oxz;
    float* tmax;
    double* w;
    const uint8_t* occluded; // the reduce kernels: the chunk's answers
    double* e_planes;        // f64[count][T]
    double* v_planes;        // f64[count][T] (the variance reduce)
    int32_t k0, lt0, pair_count;
    int32_t first_tri, tri_count, samples, T;
    int32_t mode;            // which instantiation is launched
};
void launch_gather_generate_batch(const GatherBatchParams& p, hipStream_t s);
void launch_gather_reduce_batch(const GatherBatchParams& p, bool variance, hipStream_t s);

// ---- the adaptive gather (uvrt_refine.hip; include/uvrt.h "adaptive gather") ----
// extra[t] = n_t of the count rule for t in [first_tri, first_tri + tri_count), 0 for every other t < T
void launch_refine_count(const float4* gtris, const double* expected, const double* variance, int32_t* extra, int32_t T,
                         int32_t first_tri, int32_t tri_count, int32_t samples0, double rel_error, double min_expected,
                         int32_t max_extra, hipStream_t s);
// offs[i] = extra[first_tri] + ... + extra[first_tri + i - 1] for i in [0, tri_count]; block_sums: (tri_count + 1023) / 1024
// int32 of scratch
void launch_refine_scan(const int32_t* extra, int32_t* offs, int32_t* block_sums, int32_t first_tri, int32_t tri_count,
                        hipStream_t s);
// A chunk of a refined range: the triangles first_tri + [lo, hi) and their offs[hi] - offs[lo] rays, ray r of the chunk being
// sample r + offs[lo] - offs[i] of the triangle i whose offsets enclose it.  g.samples is not read: S is the triangle's n_t.
void launch_refine_generate(const GatherGenParams& g, const int32_t* offs, int32_t lo, int32_t hi, int32_t rays, hipStream_t s);
// X1, V1 of every triangle of the chunk with n_t > 0 as k_gather_reduce_var<mode> forms them at S = n_t, merged in place
void launch_refine_reduce(const float4* gtris, const double* w, const uint8_t* occluded, const int32_t* offs, double* expected,
                          double* variance, int32_t first_tri, int32_t lo, int32_t hi, int32_t samples0, int32_t photons_equiv,
                          int32_t mode, hipStream_t s);

// ---- closest hits and the one-bounce gather (uvrt_indirect.hip; include/uvrt.h "one diffuse bounce") ----
// The closest-hit traversal's arguments: an OccludeParams with a hit record in place of the byte.  hit[i] = (dist bits, triID)
// as extend.cl leaves them for a ray whose dist is preset to tmax[i]; (tmax bits, 0xFFFFFFFF) when nothing is accepted.
struct ClosestParams {
    ExtendParams e;
    const float2* oxz;       // [n] orig.x, orig.z
    const float* tmax;       // [n]
    uint2* hit;              // [n]
};
bool launch_closest_free(const ClosestParams& p, int grid_per_cu, hipStream_t s);
struct IndirectGenParams {
    const float4* gtris;
    float4* rays;            // [tri_count * samples] dir.xyz, orig.y
    float2* oxz;             // orig.x, orig.z
    float* tmax;             // 1e30f, or 0 for a sample that is not traced
    uint32_t seed_hash;      // WangHash(seed)
    int32_t first_tri, tri_count, samples;
};
void launch_indirect_generate(const IndirectGenParams& p, hipStream_t s);
// expected[t] = (add ? expected[t] : 0) + ind[t] for t in [first_tri, first_tri + tri_count), from the chunk's hit records
struct IndirectReduceParams {
    const float4* gtris;
    const double* source;    // [T]
    const uint2* hit;        // [tri_count * samples]
    double* expected;        // [T]
    int32_t first_tri, tri_count, samples, T;
    float reflectance;
    int32_t add;
};
void launch_indirect_reduce(const IndirectReduceParams& p, hipStream_t s);
void launch_export_closest_rays(const float4* rays, const float2* oxz, const float* tmax, void* out32, int64_t count, hipStream_t s);

// ---- recorded hit links and multi-bounce gathers (uvrt_links.hip; include/uvrt.h "recorded hit links") ----
// The links are SAMPLE-major on the device: links[s * T + t], so that the 64 lanes of a wave (64 consecutive triangles) read
// 256 contiguous bytes per sample.
// links[s * T + t] = h_s or -1, for t in [first_tri, first_tri + tri_count), from a chunk's hit records (triangle-major)
struct LinksStoreParams {
    const float4* gtris;
    const uint2* hit;        // [tri_count * samples]
    int32_t* links;          // [samples * T]
    int32_t first_tri, tri_count, samples, T;
};
void launch_links_store(const LinksStoreParams& p, hipStream_t s);
// e[h] = nn_h > 0 ? source[h] / (0.5 * nn_h) : 0.0 for all h < T
void launch_links_irradiance(const float4* gtris, const double* source, double* e, int32_t T, hipStream_t s);
// One bounce b of uvrt_gather_indirect_linked for t in [first_tri, first_tri + tri_count): g = the lookup-and-sum over e_in.
// e_out (not the last bounce): e_out[t] = g's irradiance.  total_in / total_out: the running sum g_1 + .. (null: none / not
// kept).  expected (the last bounce): expected[t] = (add ? expected[t] : 0) + total.
struct LinksApplyParams {
    const float4* gtris;
    const int32_t* links;    // [samples * T]
    const double* e_in;      // [T]
    double* e_out;           // [T] or null
    const double* total_in;  // [T] or null (bounce 1)
    double* total_out;       // [T] or null (the last bounce)
    double* expected;        // [T] or null (every bounce but the last)
    int32_t first_tri, tri_count, samples, T;
    float reflectance;
    int32_t add;
};
void launch_links_apply(const LinksApplyParams& p, hipStream_t s);
// the sided forms (include/uvrt.h "face-resolved gather and bounces").  The store: links[s * T + t] =
// (h_s << 1) | a_s or -1, a_s the face of h_s the chunk's ray (rays: lane 0's, dir.xyz as the generate kernel wrote them)
// arrives on.  The irradiance: e[2 * h + f] = nn_h > 0 ? faces[f * T + h] / (0.5 * nn_h) : 0.0, interleaved so that a sided link
// is the index of what it points at.  The apply: LinksApplyParams with e_in / e_out of 2 * T entries; sample s leaves face
// s & 1 of t, g[f] sums the samples of face f and the total takes g[0] + g[1].
void launch_links_store_sided(const LinksStoreParams& p, const float4* rays, hipStream_t s);
void launch_links_irradiance_sided(const float4* gtris, const double* faces, double* e, int32_t T, hipStream_t s);
void launch_links_apply_sided(const LinksApplyParams& p, hipStream_t s);
// the mapped forms (include/uvrt.h "per-face reflectance"): rho[f * T + t], f32[2][T], the reflectance of
// face f of t.  The radiosity: r[2 * h + f] = nn_h > 0 ? (double)rho[f * T + h] * (faces[f * T + h] / (0.5 * nn_h)) : 0.0, in
// the sided irradiance's layout.  The apply: the sided apply without a reflectance on the receiver; r_out (not the last bounce)
// takes rho of t's own faces times the irradiance they have just received, the next bounce's r_in.
void launch_links_radiosity_sided(const float4* gtris, const double* faces, const float* rho, double* r, int32_t T, hipStream_t s);
struct LinksMappedParams {
    const float4* gtris;
    const int32_t* links;    // [samples * T], sided
    const float* rho;        // [2 * T]
    const double* r_in;      // [2 * T]
    double* r_out;           // [2 * T] or null (the last bounce)
    const double* total_in;  // [T] or null (bounce 1)
    double* total_out;       // [T] or null (the last bounce)
    double* expected;        // [T] or null (every bounce but the last)
    int32_t first_tri, tri_count, samples, T;
    int32_t add;
};
void launch_links_apply_mapped(const LinksMappedParams& p, hipStream_t s);
// test hook: out[(t - first_tri) * samples + s] = links[s * T + t]
void launch_links_export(const int32_t* links, int32_t* out, int32_t first_tri, int32_t tri_count, int32_t samples, int32_t T,
                         hipStream_t s);

// ---- specular panels and the mirror gather (uvrt_mirror.hip; include/uvrt.h "specular panels") ----
// A panel as the kernels read it: the plane's point and unit normal in f64 (the host normalises), the reflectance, and the
// value panel_of_tri holds for its member triangles.
struct MirrorPanel {
    double qx, qy, qz;
    double mx, my, mz;
    double rho;              // (double) of the f32 reflectance
    int32_t member;          // k + 1
    int32_t pad;
};
// leg A of every (triangle, sample) of a chunk: a GatherGenParams' arrays (w: rho * the image's weight), the face byte and
// the receiver point of each sample
struct MirrorGenParams {
    GatherGenParams g;
    MirrorPanel m;
    uint8_t* face;           // [tri_count * samples]
    float4* point;           // [tri_count * samples] p.xyz
};
void launch_mirror_generate(const MirrorGenParams& p, hipStream_t s);
// leg B over leg A, from the chunk's hit records; w[i] = 0 for a sample whose leg A did not end on the panel
struct MirrorFoldParams {
    float4* rays;
    float2* oxz;
    float* tmax;
    double* w;
    const uint2* hit;
    const float4* point;
    const uint8_t* panel_of_tri;   // [T]
    int64_t n;
    int32_t member, T;
};
void launch_mirror_fold(const MirrorFoldParams& p, hipStream_t s);
// expected[t] (and, with `faces`, faces[f * T + t]) = accumulate ? old + m : m for the chunk's triangles
struct MirrorReduceParams {
    const float4* gtris;
    const double* w;
    const uint8_t* occluded;
    const uint8_t* face;
    double* expected;        // [T]
    double* faces;           // [2 * T], or null: the faces state is off
    int32_t first_tri, tri_count, samples, photons_equiv, T;
    int32_t accumulate;
};
void launch_mirror_reduce(const MirrorReduceParams& p, hipStream_t s);

// ---- virtual dosimeters (uvrt_sensors.hip; include/uvrt.h "sensors") ----
// The sensors on the device are the caller's 32-byte records as they came, read as two float4: {pos.xyz, normal.x},
// {normal.y, normal.z, kind bits, reserved}.  The five planes are one array f64[5][K]: density, variance, dose_map, max_map,
// var_map (the `which` of uvrt_read_sensor_plane).
struct SensorGenParams {
    const float4* sensors;   // [K * 2]
    float4* rays;            // [count * samples] dir.xyz, orig.y
    float2* oxz;             // orig.x, orig.z
    float* tmax;
    double* w;               // the sample's weight (0 for a sample that is not traced); the reflected generate leaves it alone
    float fx, fy, fz, tx, ty, tz;
    float light_length;
    uint32_t seed_hash;      // WangHash(seed)
    int32_t first, count, samples;
    uint32_t seed;           // the raw seed (the stratified rule's rotation)
    int32_t mode;            // UVRT_GATHER_INDEPENDENT / UVRT_GATHER_STRATIFIED: which instantiation is launched
};
void launch_sensor_generate(const SensorGenParams& p, hipStream_t s);
void launch_sensor_indirect_generate(const SensorGenParams& p, hipStream_t s);
// density[k] and variance[k] of the chunk's sensors from its weights and answers
struct SensorReduceParams {
    const double* w;
    const uint8_t* occluded;
    double* density;         // [K]
    double* variance;        // [K]
    int32_t first, count, samples, photons_equiv;
    int32_t mode;
};
void launch_sensor_reduce(const SensorReduceParams& p, hipStream_t s);
// density[k] += the reflected part of the chunk's sensors, from its hit records (and, emitter 1, its rays' directions)
struct SensorIndirectReduceParams {
    const float4* sensors;
    const float4* gtris;
    const float4* rays;
    const uint2* hit;
    const double* source;    // [T] (emitter 0)
    const double* faces;     // [2 * T] (emitter 1)
    const float* rho;        // [2 * T] (use_map) or null
    double* density;         // [K]
    int32_t first, count, samples, T;
    float reflectance;
    int32_t emitter, use_map;
};
void launch_sensor_indirect_reduce(const SensorIndirectReduceParams& p, hipStream_t s);
// accumulate.cl's rule per sensor over planes f64[5][K]; out[k] = k_compute_dosage's value of map[first + k] with area 1.0f
void launch_sensor_accumulate(double* planes, int32_t K, float time_step, hipStream_t s);
void launch_sensor_dosage(const double* map, float* out, int32_t photons_per_light, float scaled_power, int32_t first, int32_t count,
                          hipStream_t s);

}  // namespace uvrt

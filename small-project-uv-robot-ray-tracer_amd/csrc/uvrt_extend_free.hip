// uvrt_extend_free.hip -- extend (cl/extend.cl:6-99) for rays that each carry their own origin, the sweep generator that
// makes such rays (a lamp that radiates while it moves), and their export.
//
// k_extend6 (uvrt_extend6.hip) traces the rays of ONE lamp column: the x / z slab numerators b - o come out of per-launch
// records with the lamp's x / z already subtracted.  k_extend_free is the same persistent-wave traversal -- statically owned
// 64-ray batches, in-wave refill, one step per lane and trip, the reference's BVH2 visit order (extend.cl:40-81), leaf visits
// in every second trip, the LDS stack with its global overflow rows -- for rays of any origin:
//
//  * the lane state (uvrt_traverse.h LaneF) holds {orig.x, orig.z} beside {orig.y, dist}; the refill reads them from a second
//    ray array;
//  * the records are the scene's own ("free records": prepare_record6's layout with the raw bounds, made once per scene,
//    breadth-first), so no launch prepares anything; a step forms a = b - o for x and z as it always did for y, one
//    v_pk_add_f32 with a negated, broadcast origin per (min, max) pair -- the same single f32 subtraction as extend.cl:31,35;
//  * the first levels of the tree (uvrt_set_scene's breadth-first prefix, <= 175 records) are served from LDS;
//  * everything else is uvrt_traverse.h's, the same functions k_extend6 calls: the refill (refill_lane), the step (step6 /
//    step7, which subtract a LaneF's own x / z origin where Lane6's records come with it subtracted), the box and triangle
//    tests and the deposit.  This file holds the kernel's loop, the launch wrappers, the generators and the export.
// Batched tracing (include/uvrt.h uvrt_trace_batch_launches) runs the instantiations with PLANES: the launch holds the planes of
// several sweeps side by side, as k_extend6 holds those of several stops, and k_generate_sweep_batch makes their rays.
// The trips are hipcc's code for the lane-mask form of the step (step7), not k_extend6's hand-written stream; a trip with a
// lane that needs IEEE divisions or whose stack has left LDS takes the general step (step6).
//
// Why the packed division covers numerators formed per ray.  slabs6 computes q = RN(a / d) as q0 = a * y, r = fma(-d, q0, a),
// q = fma(r, y, q0) with y = RN(1 / d).  That this equals the IEEE quotient for every pair of significands was shown by
// exhaustion (tests/tools/div3_exhaustive.hip); what is left is the exponents -- no step may overflow, and q0 and r must
// not lose bits below the normal range.  k_extend6 bounds them with three conditions: 2^-60 <= |d| <= 1
// (outside_proof_conditions), every box bound zero or in [2^-60, 1e9] (uvrt_set_scene: scene_force_exact), every origin
// component zero or in [2^-100, 1e9] (the ray's y per ray, the lamp's x / z per launch: variant_force_exact).  Its y
// numerators are already formed per ray in the step, a = RN(b - o.y), from exactly these bounds and this window; the x / z
// numerators here are the same expression of the same bounds and an origin component under the same window, so they
// lie in the range the y numerators have, and the argument that covers y there covers x and z here.  refill_lane
// therefore tests a LaneF's orig.x and orig.z (origin_outside_window) as outside_proof_conditions tests orig.y.  A ray that
// fails (a NaN or infinite origin component fails the range test too) takes the exact step, IEEE divisions as the reference
// writes them.  The launch-uniform conditions stay what they were: scene_force_exact and variants 500-599 put every ray on
// the exact step.
#include "uvrt_query.h"

namespace uvrt {

// PLANES: the launch holds the planes of a batch (uvrt_trace_batch_launches), one count plane per sweep; a batch never
// records hits, so PLANES comes with RECORD = false
template <bool RECORD, int FL, bool PLANES>
__global__ __launch_bounds__(256, FREE_GRID_PER_CU) void k_extend_free(FreeParams fp)
{
    static_assert(FL == 0 || FL == 1, "free rays: flavours 0 and 1");
    const ExtendParams& p = fp.e;
    __shared__ __attribute__((aligned(1024))) uint32_t s_stack[PS6 + 1][256];   // row 0 always holds REF_DONE ("entry -1")
    __shared__ float4 s_top[(TOP6_MAX + 1) * (TOP6_STRIDE / 16)];
    const uint32_t top_pairs = p.top_pairs < TOP6_MAX ? p.top_pairs : TOP6_MAX;
    {
        const float4* src = (const float4*)p.recs;
        for (uint32_t i = threadIdx.x; i < top_pairs * 4u; i += 256u) s_top[i] = src[i];
    }
    s_stack[0][threadIdx.x] = REF_DONE;
    __syncthreads();
    const uint32_t stack_base = (uint32_t)(uintptr_t)&s_stack[0][threadIdx.x];
    LaneF L;
    L.px = L.py = L.pz = (v2f){1.f, 1.f};
    L.po = (v2f){0.f, 1e30f};      // dist == 1e30f <=> nothing to deposit
    L.oxz = (v2f){0.f, 0.f};
    L.triID = 0;
    L.cur = REF_DONE;
    L.sp = 0;
    uint32_t slot = 0;
    bool live = false;
    int32_t* const my_counts = p.counts + (int64_t)(blockIdx.x % (unsigned)p.count_replicas) * p.count_stride;
    uint32_t plane_off = 0;         // bit 31: the lane's ray needs the exact step; PLANES: below it, ints to the ray's plane
    const uint32_t wave = blockIdx.x * 4u + (uint32_t)__builtin_amdgcn_readfirstlane(threadIdx.x >> 6);
    const uint32_t W = gridDim.x * 4u;
    uint32_t cursor = 0;
    const uint32_t chunk_end = p.chunk;
    unsigned long long km = ~0ull;          // all ones in a trip that visits leaves (every second one)
    unsigned long long full;
    asm volatile("s_mov_b64 %0, exec" : "=s"(full));
    const uint32_t top_base = (uint32_t)(uintptr_t)s_top;
    int refill_at = p.refill_min;           // idle lanes that trigger a refill; 64 once the wave's share is handed out

    for (;;) {
        const unsigned long long special_mask = __builtin_amdgcn_ballot_w64((int32_t)plane_off < 0);
        const unsigned long long idle_mask = __builtin_amdgcn_ballot_w64(L.cur == REF_DONE);
        const int nidle = __popcll(idle_mask);
        if (nidle >= refill_at) {
            if (cursor < chunk_end) {
                if (L.cur == REF_DONE) refill_lane<RECORD, FL, PLANES ? PLANES_ALL : PLANES_NONE>(L, p, fp.oxz, my_counts, plane_off, slot, live, idle_mask, cursor, wave, W, p.root_ref6);
                cursor += (uint32_t)nidle;
                if (cursor >= chunk_end) refill_at = 64;
            }
            if (__builtin_amdgcn_ballot_w64(L.cur != REF_DONE) == 0) {
                if (cursor >= chunk_end) break;
                continue;
            }
        }
        const unsigned long long m_in = __builtin_amdgcn_ballot_w64((int32_t)L.cur >= 0);
        const unsigned long long m_lf = __builtin_amdgcn_ballot_w64((int32_t)L.cur < -1);
        const unsigned long long m_top = __builtin_amdgcn_ballot_w64(L.cur < top_pairs);
        const unsigned long long m_deep = __builtin_amdgcn_ballot_w64(L.sp >= PS6);
        // leaves are visited in every second trip, and in any trip that has no lane at an inner node
        const unsigned long long kme = m_in == 0 ? ~0ull : km;
        km = ~km;
        if ((special_mask | m_deep) != 0)
            step6<true, FL>(L, p, stack_base, s_top, top_pairs, kme != 0, (special_mask & (m_in | m_lf)) != 0, m_in | m_lf);
        else
            step7<true, FL>(L, p, stack_base, top_base, m_in, m_lf & kme, m_top, full);
    }
    retire_ray<RECORD>(L, p, my_counts, plane_off, slot, live);
}

// free records [0, P): prepare_record6 without a lamp and without a renumbering
__global__ __launch_bounds__(256) void k_prepare_free_records(const PairRec* __restrict__ pairs, float4* __restrict__ recs, int32_t npairs)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= npairs) return;
    const PairRec pr = pairs[i];
    uint32_t r0 = __float_as_uint(pr.c0min_ref0.w), r1 = __float_as_uint(pr.c0max_ref1.w);
    if (r0 >= REF_LEAF_BIT) r0 += (uint32_t)npairs;
    if (r1 >= REF_LEAF_BIT) r1 += (uint32_t)npairs;
    recs[i * 4 + 0] = make_float4(pr.c0min_ref0.x, pr.c0max_ref1.x, pr.c0min_ref0.z, pr.c0max_ref1.z);
    recs[i * 4 + 1] = make_float4(pr.c1min.x, pr.c1max.x, pr.c1min.z, pr.c1max.z);
    recs[i * 4 + 2] = make_float4(pr.c0min_ref0.y, pr.c0max_ref1.y, pr.c1min.y, pr.c1max.y);
    recs[i * 4 + 3] = make_float4(__uint_as_float(r0), __uint_as_float(r1), 0.f, 0.f);
}

void launch_prepare_free_records(const PairRec* pairs, const LeafTri* ltris, void* recs, int32_t npairs, int32_t T, hipStream_t s)
{
    if (npairs > 0)
        hipLaunchKernelGGL(k_prepare_free_records, dim3((unsigned)((npairs + 255) / 256)), dim3(256), 0, s, pairs, (float4*)recs, npairs);
    launch_prepare_leaves6(ltris, recs, npairs, T, s);
}

// One dispatch for both kinds of free launch: the persistent grid, the root reference, the instantiation.  false (nothing
// launched): a flavour the free kernel does not have, or a grid whose overflow stacks would not fit.
static bool dispatch_extend_free(FreeParams& fp, bool planes, int grid_per_cu, hipStream_t s)
{
    ExtendParams& p = fp.e;
    const unsigned grid = prepare_free_launch(p, grid_per_cu);
    if (grid == 0) return false;
#define UVRT_LFK(REC, PL)                                                                                              \
    do {                                                                                                               \
        if (p.flavour == 1) hipLaunchKernelGGL((k_extend_free<REC, 1, PL>), dim3(grid), dim3(256), 0, s, fp);           \
        else hipLaunchKernelGGL((k_extend_free<REC, 0, PL>), dim3(grid), dim3(256), 0, s, fp);                          \
    } while (0)
    if (planes) UVRT_LFK(false, true);
    else if (p.hits) UVRT_LFK(true, false);
    else UVRT_LFK(false, false);
#undef UVRT_LFK
    return true;
}

bool launch_extend_free(const FreeParams& p0, int grid_per_cu, hipStream_t s)
{
    if (p0.e.n <= 0) return true;
    FreeParams fp = p0;
    fp.e.plane_batches = 0;                 // one launch, one plane
    return dispatch_extend_free(fp, false, grid_per_cu, s);
}

bool launch_extend_free_planes(const FreeParams& p0, int grid_per_cu, hipStream_t s)
{
    if (p0.e.n <= 0) return true;
    FreeParams fp = p0;
    if (fp.e.plane_batches == 0 || fp.e.plane_stride == 0 || fp.e.hits) return false;
    return dispatch_extend_free(fp, true, grid_per_cu, s);
}

// ---- a lamp that moves: generate.cl:13-35 at `from`, then one more draw u for the place on the segment ----
// orig = generate's origin + u (to - from), each component fl(a + fl(u * fl(b - a))) (this file is built without contraction)
__global__ __launch_bounds__(256) void k_generate_sweep(SweepParams p)
{
    helper_priority(p.prio);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    float r0;
    double x, y;
    uint32_t seed;
    const float4 ray = generate_ray_rng(p.fx, p.fy, p.fz, p.light_length, p.first_gid + i, p.seed_prev, p.seed_next, 0, r0, x, y, seed);
    const float u = random_float(seed);
    const float dx = p.tx - p.fx, dy = p.ty - p.fy, dz = p.tz - p.fz;
    const float ux = u * dx, uy = u * dy, uz = u * dz;
    p.rays[i] = make_float4(ray.x, ray.y, ray.z, ray.w + uy);
    p.oxz[i] = make_float2(p.fx + ux, p.fz + uz);
}

void launch_generate_sweep(const SweepParams& p, hipStream_t s)
{
    if (p.n <= 0) return;
    hipLaunchKernelGGL(k_generate_sweep, dim3((unsigned)((p.n + 255) / 256)), dim3(256), 0, s, p);
}

// k_generate_sweep for the sweeps of a batch: blockIdx.y is the plane, the arithmetic is the same
__global__ __launch_bounds__(256) void k_generate_sweep_batch(SweepBatchParams p)
{
    helper_priority(p.prio);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int k = blockIdx.y;
    const float fx = p.fx[k], fy = p.fy[k], fz = p.fz[k];
    float r0;
    double x, y;
    uint32_t seed;
    const float4 ray = generate_ray_rng(fx, fy, fz, p.light_length, p.first_gid + i, p.seed_prev[k], p.seed_next[k], 0, r0, x, y, seed);
    const float u = random_float(seed);
    const float dx = p.tx[k] - fx, dy = p.ty[k] - fy, dz = p.tz[k] - fz;
    const float ux = u * dx, uy = u * dy, uz = u * dz;
    const int64_t at = (int64_t)k * p.n_pad + i;
    p.rays[at] = make_float4(ray.x, ray.y, ray.z, ray.w + uy);
    p.oxz[at] = make_float2(fx + ux, fz + uz);
}

void launch_generate_sweep_batch(const SweepBatchParams& p, hipStream_t s)
{
    if (p.n <= 0 || p.count <= 0) return;
    hipLaunchKernelGGL(k_generate_sweep_batch, dim3((unsigned)((p.n + 255) / 256), (unsigned)p.count), dim3(256), 0, s, p);
}

// Test hook: the reference's 32-byte Ray records in gid order, every ray with its own origin
__global__ __launch_bounds__(256) void k_export_free_rays(const float4* __restrict__ rays, const float2* __restrict__ oxz,
                                                          const uint2* __restrict__ hits, float4* __restrict__ out,
                                                          int64_t first, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float4 rec = rays[first + i];
    const float2 o = oxz[first + i];
    uint2 h = make_uint2(__float_as_uint(1e30f), 0u);
    if (hits) h = hits[first + i];
    out[i * 2 + 0] = make_float4(rec.x, rec.y, rec.z, o.x);
    out[i * 2 + 1] = make_float4(rec.w, o.y, __uint_as_float(h.x), __uint_as_float(h.y));
}

void launch_export_free_rays(const float4* rays, const float2* oxz, const uint2* hits, void* out32, int64_t first,
                             int64_t count, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_export_free_rays, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, rays, oxz, hits,
                       (float4*)out32, first, count);
}

}  // namespace uvrt

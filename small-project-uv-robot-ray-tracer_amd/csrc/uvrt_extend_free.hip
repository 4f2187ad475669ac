// uvrt_extend_free.hip -- extend (cl/extend.cl:6-99) for rays that each carry their own origin, the sweep generator that
// makes such rays (a lamp that radiates while it moves), and their export.
//
// k_extend6 (uvrt_extend6.hip) traces the rays of ONE lamp column: the x / z slab numerators b - o come out of per-launch
// records with the lamp's x / z already subtracted.  k_extend_free is the same persistent-wave traversal -- statically owned
// 64-ray batches, in-wave refill, one step per lane and trip, the reference's BVH2 visit order (extend.cl:40-81), leaf visits
// in every second trip, the LDS stack with its global overflow rows -- for rays of any origin:
//
//  * the lane state holds {orig.x, orig.z} beside {orig.y, dist}; the refill reads them from a second ray array;
//  * the records are the scene's own ("free records": prepare_record6's layout with the raw bounds, made once per scene,
//    breadth-first), so no launch prepares anything; a step forms a = b - o for x and z as it always did for y, one
//    v_pk_add_f32 with a negated, broadcast origin per (min, max) pair -- the same single f32 subtraction as extend.cl:31,35;
//  * the first levels of the tree (uvrt_set_scene's breadth-first prefix, <= 175 records) are served from LDS;
//  * the box test, the triangle test and the deposit are uvrt_traverse.h's: slabs6 / box2_fast / box_fast / box_exact / tri6 /
//    retire_ray.
// Batched tracing (include/uvrt.h uvrt_trace_batch_launches) runs the instantiations with PLANES: the launch holds the planes of
// several sweeps side by side, as k_extend6 holds those of several stops, and k_generate_sweep_batch makes their rays.
// The trips are hipcc's code for the lane-mask form of the step (k_extend6's step7), not a hand-written stream: the general
// step (IEEE divisions, stacks beyond LDS) is k_extend6's step6 with the numerators formed per ray.
//
// Why the packed division covers numerators formed per ray.  slabs6 computes q = RN(a / d) as q0 = a * y, r = fma(-d, q0, a),
// q = fma(r, y, q0) with y = RN(1 / d).  That this equals the IEEE quotient for every pair of significands was shown by
// exhaustion (tests/tools/div3_exhaustive.hip); what is left is the exponents -- no step may overflow, and q0 and r must
// not lose bits below the normal range.  k_extend6 bounds them with three conditions: 2^-60 <= |d| <= 1
// (outside_proof_conditions), every box bound zero or in [2^-60, 1e9] (uvrt_set_scene: scene_force_exact), every origin
// component zero or in [2^-100, 1e9] (the ray's y per ray, the lamp's x / z per launch: variant_force_exact).  Its y
// numerators are already formed per ray in the step, a = RN(b - o.y), from exactly these bounds and this window; the x / z
// numerators here are the same expression of the same bounds and an origin component under the same window, so they
// lie in the range the y numerators have, and the argument that covers y there covers x and z here.  refill_free
// therefore tests orig.x and orig.z as outside_proof_conditions tests orig.y.  A ray that fails (a NaN or infinite
// origin component fails the range test too) takes the exact step, IEEE divisions as the reference writes them.  The
// launch-uniform conditions stay what they were: scene_force_exact and variants 500-599 put every ray on the exact step.
#include "uvrt_traverse.h"

namespace uvrt {

struct LaneF : Lane6 {
    v2f oxz;                // {origin x, origin z}
};

// a = b - o for the x and z (min, max) pairs of both children
__device__ __forceinline__ void sub_xz(v2f& x0, v2f& z0, v2f& x1, v2f& z1, v2f oxz)
{
    asm("v_pk_add_f32 %[x0], %[x0], %[o] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[z0], %[z0], %[o] op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[x1], %[x1], %[o] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_add_f32 %[z1], %[z1], %[o] op_sel:[0,1] op_sel_hi:[1,1] neg_lo:[0,1] neg_hi:[0,1]"
        : [x0] "+v"(x0), [z0] "+v"(z0), [x1] "+v"(x1), [z1] "+v"(z1)
        : [o] "v"(oxz));
}

// |o| zero or in [2^-100, 1e9]: the window outside_proof_conditions applies to the origin's y
__device__ __forceinline__ bool origin_outside_window(float o)
{
    const uint32_t uo = __float_as_uint(o) & 0x7FFFFFFFu;
    const uint32_t lo = 0x0D800000u /* 2^-100 */, hi = 0x4E6E6B28u /* 1e9f */;
    return uo != 0u && uo - lo > hi - lo;
}

// refill_lane (uvrt_traverse.h) for a launch of free rays: gid order, the origin's x / z from their own array.
// PLANES: the launch holds the planes of a batch -- the plane of the lane's 64-slot batch and its padding as refill_lane
// finds them, the plane's offset beside the exact-step bit in plane_off.
template <bool RECORD, bool PLANES>
__device__ __forceinline__ void refill_free(LaneF& L, const FreeParams& fp, int32_t* my_counts, uint32_t& plane_off,
                                            uint32_t& slot, bool& live, unsigned long long idle_mask, uint32_t cursor,
                                            uint32_t wave, uint32_t W, uint32_t root)
{
    const ExtendParams& p = fp.e;
    retire_ray<RECORD>(L, p, my_counts, plane_off, slot, live);
    live = false;
    L.po.y = 1e30f;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_mask, 0u));
    const uint32_t v = cursor + rank;
    const uint32_t gb = (v >> 6) * W + wave;                 // global 64-slot batch
    const uint32_t my = gb * 64u + (v & 63u);
    uint32_t pl = 0;
    bool in_plane = true;
    if (PLANES) {           // gb / plane_batches: exact after one correction step (refill_lane)
        pl = (uint32_t)((float)gb * p.plane_inv);
        int32_t within = (int32_t)(gb - pl * p.plane_batches);
        if (within < 0) { --pl; within += (int32_t)p.plane_batches; }
        else if ((uint32_t)within >= p.plane_batches) { ++pl; within -= (int32_t)p.plane_batches; }
        in_plane = (uint32_t)within * 64u + (v & 63u) < p.plane_n;
    }
    if (v < p.chunk && my < (uint32_t)p.n && in_plane) {
        const float4 rec = p.rays[my];
        const float2 o = fp.oxz[my];
        set_in_place(L.px, rec.x, rcp_exact(rec.x));       // y = RN32(1/d); lanes outside its range are `spec` and never use it
        set_in_place(L.py, rec.y, rcp_exact(rec.y));
        set_in_place(L.pz, rec.z, rcp_exact(rec.z));
        set_in_place(L.po, rec.w, 1e30f);
        set_in_place(L.oxz, o.x, o.y);
        set_in_place(L.triID, 0u);
        if (RECORD) { slot = my; live = true; }
        set_in_place(L.sp, 0);
        set_in_place(L.cur, root);
        const bool spec = outside_proof_conditions(rec) || origin_outside_window(o.x) || origin_outside_window(o.y) ||
                          p.force_exact != 0;
        set_in_place(plane_off, (PLANES ? pl * p.plane_stride : 0u) | (spec ? SPECIAL6 : 0u));
    }
}

// The general step (k_extend6's step6): any mix of lanes, stacks beyond LDS, and -- `exact`, wave-uniform -- the IEEE-division
// form of the box and triangle arithmetic.
template <int FL>
__device__ __forceinline__ void step_free_general(LaneF& L, const ExtendParams& p, uint32_t stack_base, const float4* s_top,
                                                  uint32_t top_pairs, bool leaf_trip, bool exact, unsigned long long m_act)
{
    const uint32_t cur = L.cur;
    const bool is_inner = cur < REF_LEAF_BIT;
    const bool is_leaf = (cur >= REF_LEAF_BIT) & (cur != REF_DONE) & leaf_trip;
    const uint32_t idx = cur & REF_FIRST_MASK;
    v4f w0, w1, w2, w3;
    uint32_t spec_top = REF_DONE;                       // stays REF_DONE when the stack is empty
    const uint32_t sa = stack_base + ((uint32_t)L.sp << 10);
    {
        const unsigned long long m_in = __builtin_amdgcn_ballot_w64(cur < REF_LEAF_BIT);
        const unsigned long long m_top = __builtin_amdgcn_ballot_w64(cur < top_pairs);
        const unsigned long long m_sp = __builtin_amdgcn_ballot_w64(L.sp > 0);
        const unsigned long long m_go = m_in | (leaf_trip ? (m_act & ~m_in) : 0ull);
        const unsigned long long m_glob = m_go & ~m_top;
        const unsigned long long m_stk = m_go & m_sp;
        const uint32_t a0 = (uint32_t)(uintptr_t)s_top + cur * TOP6_STRIDE;
        const uint32_t roff = cur << 6;
        unsigned long long save;
        asm volatile("s_mov_b64 %[save], exec\n\t"
                     "s_mov_b64 exec, %[mstk]\n\t"
                     "ds_read_b32 %[st], %[sa]\n\t"
                     "s_mov_b64 exec, %[mtop]\n\t"
                     "ds_read_b128 %[w0], %[a0]\n\t"
                     "ds_read_b128 %[w1], %[a0] offset:16\n\t"
                     "ds_read_b128 %[w2], %[a0] offset:32\n\t"
                     "ds_read_b128 %[w3], %[a0] offset:48\n\t"
                     "s_mov_b64 exec, %[mglob]\n\t"
                     "global_load_dwordx4 %[w0], %[ro], %[rb]\n\t"
                     "global_load_dwordx4 %[w1], %[ro], %[rb] offset:16\n\t"
                     "global_load_dwordx4 %[w2], %[ro], %[rb] offset:32\n\t"
                     "global_load_dwordx4 %[w3], %[ro], %[rb] offset:48\n\t"
                     "s_mov_b64 exec, %[save]\n\t"
                     "s_waitcnt vmcnt(0) lgkmcnt(0)"
                     : [w0] "=&v"(w0), [w1] "=&v"(w1), [w2] "=&v"(w2), [w3] "=&v"(w3), [st] "+v"(spec_top),
                       [save] "=&s"(save)
                     : [a0] "v"(a0), [sa] "v"(sa), [ro] "v"(roff), [rb] "s"(p.recs),
                       [mtop] "s"(m_top), [mglob] "s"(m_glob), [mstk] "s"(m_stk)
                     : "memory");
    }
    bool need_pop = is_leaf;
    if (is_inner) {
        float d0, d1;
        bool h0, h1;
        const float ox = L.oxz.x, oy = L.po.x, oz = L.oxz.y;
        if (exact) {
            h0 = box_exact(w0.x - ox, w0.y - ox, w2.x - oy, w2.y - oy, w0.z - oz, w0.w - oz, L.px.x, L.py.x, L.pz.x, L.po.y, d0);
            h1 = box_exact(w1.x - ox, w1.y - ox, w2.z - oy, w2.w - oy, w1.z - oz, w1.w - oz, L.px.x, L.py.x, L.pz.x, L.po.y, d1);
        } else {
            v2f x0 = __builtin_shufflevector(w0, w0, 0, 1), z0 = __builtin_shufflevector(w0, w0, 2, 3);
            v2f x1 = __builtin_shufflevector(w1, w1, 0, 1), z1 = __builtin_shufflevector(w1, w1, 2, 3);
            v2f y0 = __builtin_shufflevector(w2, w2, 0, 1), y1 = __builtin_shufflevector(w2, w2, 2, 3);
            sub_xz(x0, z0, x1, z1, L.oxz);
            slabs6(x0, y0, z0, L.px, L.py, L.pz, L.po);
            h0 = box_fast(x0, y0, z0, L.po.y, d0);
            slabs6(x1, y1, z1, L.px, L.py, L.pz, L.po);
            h1 = box_fast(x1, y1, z1, L.po.y, d1);
        }
        // extend.cl:56-76: child 1 first iff it is hit and child 0 is missed or farther; both hit: the farther is pushed
        const bool sw = h1 & (!h0 | (d0 > d1));
        const uint32_t r0 = __float_as_uint(w3.x), r1 = __float_as_uint(w3.y);
        const uint32_t nearer = sw ? r1 : r0, farther = sw ? r0 : r1;
        if (h0 & h1) {
            if (L.sp < PS6) asm volatile("ds_write_b32 %0, %1 offset:1024" : : "v"(sa), "v"(farther) : "memory");
            else if (L.sp < MAXS6) ovf_ptr(p, stack_base)[L.sp - PS6] = farther;
            else *p.error_flag = 1u;
            L.sp = L.sp < MAXS6 ? L.sp + 1 : L.sp;
        }
        need_pop = !(h0 | h1);
        L.cur = nearer;
    }
    if (is_leaf) {                                       // extend.cl:48-55
        uint32_t count = (cur >> REF_COUNT_SHIFT) & 15u;
        const uint32_t first = idx - (uint32_t)p.npairs;
        if (count == 15u) count = p.scene.leaf_count[first];
        float dist = L.po.y;
        tri6<FL>(L.oxz.x, L.po.x, L.oxz.y, L.px.x, L.py.x, L.pz.x, dist, L.triID,
                 make_float4(w0.x, w0.y, w0.z, w0.w), make_float4(w1.x, w1.y, w1.z, w1.w),
                 make_float4(w2.x, w2.y, w2.z, w2.w), exact);
        for (uint32_t i = 1; i < count; ++i) {
            const float4* lt = (const float4*)p.recs + ((size_t)idx + i) * 4;
            tri6<FL>(L.oxz.x, L.po.x, L.oxz.y, L.px.x, L.py.x, L.pz.x, dist, L.triID, lt[0], lt[1], lt[2], exact);
        }
        L.po.y = dist;
    }
    if (need_pop) {
        uint32_t popped = spec_top;                        // REF_DONE when the stack is empty
        if (L.sp > PS6) popped = ovf_ptr(p, stack_base)[L.sp - 1 - PS6];
        L.cur = popped;
        L.sp = (int)__builtin_elementwise_sub_sat((uint32_t)L.sp, 1u);
    }
}

// The common trip (k_extend6's step7): no lane needs the IEEE-division form, no lane's stack has left LDS; the control flow
// as lane masks.  m_in: lanes at an inner node, m_leaf: lanes that visit their leaf in this trip, m_top: lanes whose record is
// in the LDS cache, full: the exec mask of the loop (all 64 lanes).
template <int FL>
__device__ __forceinline__ void step_free(LaneF& L, const ExtendParams& p, uint32_t stack_base, uint32_t top_base,
                                          unsigned long long m_in, unsigned long long m_leaf, unsigned long long m_top,
                                          unsigned long long full)
{
    const uint32_t cur = L.cur;
    v4f w0, w1, w2, w3;
    uint32_t spec_top;
    const uint32_t sa = stack_base + ((uint32_t)L.sp << 10);
    {
        const unsigned long long m_glob = (m_in | m_leaf) & ~m_top;
        const uint32_t a0 = __umul24(cur, TOP6_STRIDE) + top_base;      // only used by lanes in m_top
        const uint32_t roff = cur << 6;
        // the stack top is read by every lane: entry -1 of a lane's LDS stack is a row that always holds REF_DONE
        asm volatile("ds_read_b32 %[st], %[sa]\n\t"
                     "s_mov_b64 exec, %[mtop]\n\t"
                     "ds_read_b128 %[w0], %[a0]\n\t"
                     "ds_read_b128 %[w1], %[a0] offset:16\n\t"
                     "ds_read_b128 %[w2], %[a0] offset:32\n\t"
                     "ds_read_b128 %[w3], %[a0] offset:48\n\t"
                     "s_mov_b64 exec, %[mglob]\n\t"
                     "global_load_dwordx4 %[w0], %[ro], %[rb]\n\t"
                     "global_load_dwordx4 %[w1], %[ro], %[rb] offset:16\n\t"
                     "global_load_dwordx4 %[w2], %[ro], %[rb] offset:32\n\t"
                     "global_load_dwordx4 %[w3], %[ro], %[rb] offset:48\n\t"
                     "s_mov_b64 exec, %[full]\n\t"
                     "s_waitcnt vmcnt(0) lgkmcnt(0)"
                     : [w0] "=&v"(w0), [w1] "=&v"(w1), [w2] "=&v"(w2), [w3] "=&v"(w3), [st] "=&v"(spec_top)
                     : [a0] "v"(a0), [sa] "v"(sa), [ro] "v"(roff), [rb] "s"(p.recs), [mtop] "s"(m_top), [mglob] "s"(m_glob),
                       [full] "s"(full)
                     : "memory");
    }
    if (m_leaf != 0) {                                       // wave-uniform; m_leaf != 0 means: a leaf trip
        if ((int32_t)cur < -1) {                             // at a leaf (REF_DONE is -1): extend.cl:48-55
            const uint32_t idx = cur & REF_FIRST_MASK;
            uint32_t count = (cur >> REF_COUNT_SHIFT) & 15u;
            const uint32_t first = idx - (uint32_t)p.npairs;
            if (count == 15u) count = p.scene.leaf_count[first];
            float dist = L.po.y;
            tri6<FL>(L.oxz.x, L.po.x, L.oxz.y, L.px.x, L.py.x, L.pz.x, dist, L.triID,
                     make_float4(w0.x, w0.y, w0.z, w0.w), make_float4(w1.x, w1.y, w1.z, w1.w),
                     make_float4(w2.x, w2.y, w2.z, w2.w), false);
            for (uint32_t i = 1; i < count; ++i) {
                const float4* lt = (const float4*)p.recs + ((size_t)idx + i) * 4;
                tri6<FL>(L.oxz.x, L.po.x, L.oxz.y, L.px.x, L.py.x, L.pz.x, dist, L.triID, lt[0], lt[1], lt[2], false);
            }
            L.po.y = dist;
        }
    }
    if (m_in != 0) {            // wave-uniform: a trip with no lane at an inner node skips the box arithmetic
        v2f x0 = __builtin_shufflevector(w0, w0, 0, 1), z0 = __builtin_shufflevector(w0, w0, 2, 3);
        v2f x1 = __builtin_shufflevector(w1, w1, 0, 1), z1 = __builtin_shufflevector(w1, w1, 2, 3);
        v2f y0 = __builtin_shufflevector(w2, w2, 0, 1), y1 = __builtin_shufflevector(w2, w2, 2, 3);
        sub_xz(x0, z0, x1, z1, L.oxz);
        slabs6(x0, y0, z0, L.px, L.py, L.pz, L.po);
        slabs6(x1, y1, z1, L.px, L.py, L.pz, L.po);
        float n0, f0, n1, f1;
        box2_fast(x0, y0, z0, x1, y1, z1, n0, f0, n1, f1);
        // extend.cl:36-38,56-76: hit = tmax >= tmin && tmin < dist && tmax > 0 per child; child 1 first iff it is hit
        // and child 0 is missed or farther; both hit: the farther one is pushed; none hit (or a leaf visited): pop
        unsigned long long h0, h1, t;
        asm volatile("s_mov_b64 exec, %[min]\n\t"
                     "v_cmpx_ge_f32_e64 %[h0], %[f0], %[n0]\n\t"
                     "v_cmpx_lt_f32_e64 %[h0], %[n0], %[dist]\n\t"
                     "v_cmpx_gt_f32_e64 %[h0], %[f0], 0\n\t"            // h0 = exec = inner lanes whose child 0 is hit
                     "s_mov_b64 exec, %[min]\n\t"
                     "v_cmpx_ge_f32_e64 %[h1], %[f1], %[n1]\n\t"
                     "v_cmpx_lt_f32_e64 %[h1], %[n1], %[dist]\n\t"
                     "v_cmpx_gt_f32_e64 %[h1], %[f1], 0\n\t"            // h1 likewise
                     "v_cmp_gt_f32 vcc, %[n0], %[n1]\n\t"               // (under exec = h1)
                     "s_andn2_b64 %[t], %[h1], %[h0]\n\t"
                     "s_or_b64 %[t], %[t], vcc\n\t"                     // t = child 1 first
                     "s_and_b64 exec, %[h0], %[h1]\n\t"                 // both hit: push the farther, sp + 1
                     "v_cndmask_b32 %[n1], %[r1], %[r0], %[t]\n\t"
                     "ds_write_b32 %[sa], %[n1] offset:1024\n\t"
                     "v_add_u32 %[sp], 1, %[sp]\n\t"
                     "s_or_b64 exec, %[h0], %[h1]\n\t"                  // any hit: descend into the nearer
                     "v_cndmask_b32 %[cur], %[r0], %[r1], %[t]\n\t"
                     "s_andn2_b64 %[t], %[min], exec\n\t"
                     "s_or_b64 exec, %[t], %[mleaf]\n\t"                // none hit, or a leaf was visited: pop
                     "v_mov_b32 %[cur], %[st]\n\t"
                     "v_sub_u32 %[sp], %[sp], 1 clamp\n\t"
                     "s_mov_b64 exec, %[full]"
                     : [n1] "+v"(n1), [cur] "+v"(L.cur), [sp] "+v"(L.sp), [h0] "=&s"(h0), [h1] "=&s"(h1), [t] "=&s"(t)
                     : [n0] "v"(n0), [f0] "v"(f0), [f1] "v"(f1), [dist] "v"(L.po.y), [r0] "v"(w3.x), [r1] "v"(w3.y), [sa] "v"(sa),
                       [st] "v"(spec_top), [min] "s"(m_in), [mleaf] "s"(m_leaf), [full] "s"(full)
                     : "vcc", "memory");
    } else {
        // only leaves were visited: pop them
        asm volatile("s_mov_b64 exec, %[mleaf]\n\t"
                     "v_mov_b32 %[cur], %[st]\n\t"
                     "v_sub_u32 %[sp], %[sp], 1 clamp\n\t"
                     "s_mov_b64 exec, %[full]"
                     : [cur] "+v"(L.cur), [sp] "+v"(L.sp)
                     : [st] "v"(spec_top), [mleaf] "s"(m_leaf), [full] "s"(full));
    }
}

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
                if (L.cur == REF_DONE) refill_free<RECORD, PLANES>(L, fp, my_counts, plane_off, slot, live, idle_mask, cursor, wave, W, p.root_ref6);
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
            step_free_general<FL>(L, p, stack_base, s_top, top_pairs, kme != 0, (special_mask & (m_in | m_lf)) != 0, m_in | m_lf);
        else
            step_free<FL>(L, p, stack_base, top_base, m_in, m_lf & kme, m_top, full);
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

// the persistent grid and the root reference of a free launch (0: its overflow stacks would not fit)
static unsigned size_free_launch(ExtendParams& p, int grid_per_cu)
{
    p.order = nullptr;                      // gid order
    const unsigned grid = size_persistent_grid(p, grid_per_cu < FREE_GRID_PER_CU ? grid_per_cu : FREE_GRID_PER_CU);
    p.root_ref6 = (p.scene.root_ref >= REF_LEAF_BIT && p.scene.root_ref != REF_DONE)
                      ? p.scene.root_ref + (uint32_t)p.npairs : p.scene.root_ref;
    return grid;
}

bool launch_extend_free(const FreeParams& p0, int grid_per_cu, hipStream_t s)
{
    if (p0.e.n <= 0) return true;
    FreeParams fp = p0;
    ExtendParams& p = fp.e;
    p.plane_batches = 0;                    // one launch, one plane
    const unsigned grid = size_free_launch(p, grid_per_cu);
    if (grid == 0) return false;
#define UVRT_LFK(REC, FL) hipLaunchKernelGGL((k_extend_free<REC, FL, false>), dim3(grid), dim3(256), 0, s, fp)
    if (p.flavour == 1) { if (p.hits) UVRT_LFK(true, 1); else UVRT_LFK(false, 1); }
    else if (p.flavour == 0) { if (p.hits) UVRT_LFK(true, 0); else UVRT_LFK(false, 0); }
    else return false;
#undef UVRT_LFK
    return true;
}

bool launch_extend_free_planes(const FreeParams& p0, int grid_per_cu, hipStream_t s)
{
    if (p0.e.n <= 0) return true;
    FreeParams fp = p0;
    ExtendParams& p = fp.e;
    if (p.plane_batches == 0 || p.plane_stride == 0 || p.hits) return false;
    const unsigned grid = size_free_launch(p, grid_per_cu);
    if (grid == 0) return false;
    if (p.flavour == 1) hipLaunchKernelGGL((k_extend_free<false, 1, true>), dim3(grid), dim3(256), 0, s, fp);
    else if (p.flavour == 0) hipLaunchKernelGGL((k_extend_free<false, 0, true>), dim3(grid), dim3(256), 0, s, fp);
    else return false;
    return true;
}

// ---- a lamp that moves: generate.cl:13-35 at `from`, then one more draw u for the place on the segment ----
// orig = generate's origin + u (to - from), each component fl(a + fl(u * fl(b - a))) (this file is built without contraction)
__global__ __launch_bounds__(256) void k_generate_sweep(SweepParams p)
{
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

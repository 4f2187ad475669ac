// uvrt_query.h -- the free-ray queries that deposit nothing (k_occlude_free, k_closest_free: DESIGN.md section 19), and the
// launch preparation every free-ray launch shares.
//
// run_query_rays is k_extend_free's persistent-wave traversal (uvrt_extend_free.hip) for a ray with a maximum distance and an
// answer of its own: the lane type LaneF, step6 / step7 of uvrt_traverse.h called unchanged, the same LDS top cache, stack
// and overflow rows, the same rule for the exact step.  What differs from the kernel that deposits:
//  * a refill starts a lane with dist = the ray's tmax (a third per-ray array; the lane keeps it in one register).  That is
//    what extend.cl computes when ray->dist is preset to tmax (extend.cl:25 accepts t only below dist, :36-38 culls boxes
//    beyond it);
//  * a finished ray is handed to the query's answer functor, answer(L, tmax, slot), which writes whatever the query
//    answers with.  An accepted hit shows as dist bits != tmax bits.  Bit patterns, not floats: a NaN tmax never compares
//    below anything, so it means "nothing accepted".  No deposit, no count plane, no atomics;
//  * FIRST_HIT: the first accepted hit ends the ray -- whatever is left on its stack cannot change a yes / no answer, and
//    the visit order up to it is the same.  Without it a lane runs to the end of its stack, so dist / triID end as
//    extend.cl leaves them.
// The refill is the queries' own (refill_query): refill_lane of uvrt_traverse.h stays as it is for the kernels that deposit.
// Every loop is bounded: the persistent loop by the wave's share of the rays and each ray by the reference's 32-entry stack
// (an overflow raises the error flag as in any extend).
#pragma once
#include "uvrt_traverse.h"

namespace uvrt {

constexpr uint32_t NO_SLOT = 0xFFFFFFFFu, NO_TRI = 0xFFFFFFFFu;

// What k_extend_free, k_occlude_free and k_closest_free ask of a launch before the grid exists: a flavour the free step has,
// gid order, the persistent grid and the root in the free records' numbering.  Returns the grid; 0 (launch nothing): a
// flavour other than 0 or 1, or a grid whose overflow stacks would not fit.
inline unsigned prepare_free_launch(ExtendParams& p, int grid_per_cu)
{
    if (p.flavour != 0 && p.flavour != 1) return 0;
    p.order = nullptr;                      // gid order
    const unsigned grid = size_persistent_grid(p, grid_per_cu < FREE_GRID_PER_CU ? grid_per_cu : FREE_GRID_PER_CU);
    if (grid == 0) return 0;
    p.root_ref6 = (p.scene.root_ref >= REF_LEAF_BIT && p.scene.root_ref != REF_DONE)
                      ? p.scene.root_ref + (uint32_t)p.npairs : p.scene.root_ref;
    return grid;
}

// A query launch over the n rays of qp.e: no hit records, one plane.  kernel0 / kernel1 are the query kernel's two flavours.
template <class Params>
inline bool launch_query_free(const Params& p0, void (*kernel0)(Params), void (*kernel1)(Params), int grid_per_cu, hipStream_t s)
{
    if (p0.e.n <= 0) return true;
    Params qp = p0;
    qp.e.hits = nullptr;
    qp.e.plane_batches = 0;                 // one launch, one plane
    const unsigned grid = prepare_free_launch(qp.e, grid_per_cu);
    if (grid == 0) return false;
    hipLaunchKernelGGL(qp.e.flavour == 1 ? kernel1 : kernel0, dim3(grid), dim3(256), 0, s, qp);
    return true;
}

// refill_lane (uvrt_traverse.h) for a launch without planes, hit records or deposits: the ray the lane has finished is
// answered, then the lane starts its next one at dist = tmax
template <int FL, class Answer>
__device__ __forceinline__ void refill_query(LaneF& L, const ExtendParams& p, const float2* oxz, const float* tmax_of,
                                             const Answer& answer, float& tmax, uint32_t& special, uint32_t& slot,
                                             unsigned long long idle_mask, uint32_t cursor, uint32_t wave, uint32_t W,
                                             uint32_t root)
{
    answer(L, tmax, slot);
    slot = NO_SLOT;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_mask, 0u));
    const uint32_t v = cursor + rank;
    const uint32_t gb = (v >> 6) * W + wave;                 // global 64-slot batch
    const uint32_t my = gb * 64u + (v & 63u);
    if (v < p.chunk && my < (uint32_t)p.n) {
        const float4 rec = p.rays[my];
        const float2 o = oxz[my];
        const float tm = tmax_of[my];
        set_in_place(L.px, rec.x, rcp_exact(rec.x));
        set_in_place(L.py, rec.y, rcp_exact(rec.y));
        set_in_place(L.pz, rec.z, rcp_exact(rec.z));
        set_in_place(L.po, rec.w, tm);
        set_in_place(L.oxz, o.x, o.y);
        set_in_place(tmax, tm);
        set_in_place(L.triID, 0u);
        set_in_place(slot, my);
        set_in_place(L.sp, 0);
        set_in_place(L.cur, root);
        const bool outside = outside_proof_conditions(rec) || origin_outside_window(o.x) || origin_outside_window(o.y);
        set_in_place(special, (outside || p.force_exact != 0) ? SPECIAL6 : 0u);
    }
}

// The body of a query kernel (256 threads, FREE_GRID_PER_CU workgroups per CU).  answer(L, tmax, slot) is called once for
// every ray, with slot != NO_SLOT, and for idle lanes with NO_SLOT: it tests the slot itself.
template <int FL, bool FIRST_HIT, class Answer>
__device__ __forceinline__ void run_query_rays(const ExtendParams& p, const float2* oxz, const float* tmax_of, const Answer answer)
{
    static_assert(FL == 0 || FL == 1, "free-ray queries: flavours 0 and 1");
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
    L.po = (v2f){0.f, 1e30f};
    L.oxz = (v2f){0.f, 0.f};
    L.triID = 0;
    L.cur = REF_DONE;
    L.sp = 0;
    float tmax = 1e30f;             // the bits of dist: a lane without a ray never looks finished by a hit
    uint32_t slot = NO_SLOT;
    uint32_t special = 0;           // bit 31: the lane's ray needs the exact step
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
        const unsigned long long special_mask = __builtin_amdgcn_ballot_w64((int32_t)special < 0);
        const unsigned long long idle_mask = __builtin_amdgcn_ballot_w64(L.cur == REF_DONE);
        const int nidle = __popcll(idle_mask);
        if (nidle >= refill_at) {
            if (cursor < chunk_end) {
                if (L.cur == REF_DONE) refill_query<FL>(L, p, oxz, tmax_of, answer, tmax, special, slot, idle_mask, cursor, wave, W, p.root_ref6);
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
        if (FIRST_HIT && __float_as_uint(L.po.y) != __float_as_uint(tmax)) {    // an accepted hit ends the ray
            L.cur = REF_DONE;
            L.sp = 0;
        }
    }
    answer(L, tmax, slot);
}

}  // namespace uvrt

// uvrt_indirect.hip -- the closest-hit query that deposits nothing, and the one-bounce final gather built on it
// (include/uvrt.h "one diffuse bounce").
//
// k_closest_free is k_occlude_free's persistent-wave traversal (uvrt_occlude.hip), itself k_extend_free's: the lane type
// LaneF, step6 / step7 of uvrt_traverse.h called unchanged, the same LDS top cache, stack and overflow rows, the same rule for
// the exact step.  Against k_occlude_free two things differ:
//  (a) a lane is NOT ended by its first accepted hit: it runs to the end of its stack, so dist / triID end as extend.cl
//      leaves them for a ray whose dist is preset to tmax (extend.cl:25 accepts t only below dist, :36-38 culls boxes beyond it);
//  (b) retiring writes hit[slot] = (dist bits, dist bits == tmax bits ? 0xFFFFFFFF : triID).  Bit patterns, not floats: a NaN
//      tmax never compares below anything, so it means "no hit".  No deposit, no count plane, no atomics.
// The refill and the retire are this kernel's own: uvrt_traverse.h, uvrt_extend_free.hip and uvrt_occlude.hip stay as they are.
// Every loop is bounded: the persistent loop by the wave's share of the rays and each ray by the reference's 32-entry stack
// (an overflow raises the error flag as in any extend), the disc rejection below by 8 rounds, the reduction by S2.
//
// The bounce: k_indirect_generate makes, for every (triangle, sample), a point on the triangle and a cosine-distributed
// direction about its normal (even samples leave one face, odd samples the other); k_closest_free finds what each ray sees;
// k_indirect_reduce looks up the source plane at the hit triangles and sums per triangle in sample order.  No atomics: the
// plane is a pure function of the arguments.  Only + - * / sqrt: this file is built without contraction, every operator
// below is one rounding.
#include "uvrt_traverse.h"

namespace uvrt {

constexpr uint32_t NO_SLOT = 0xFFFFFFFFu, NO_TRI = 0xFFFFFFFFu;

// the answer of the ray a lane has finished
__device__ __forceinline__ void retire_closest(const LaneF& L, const ClosestParams& cp, float tmax, uint32_t slot)
{
    if (slot != NO_SLOT) {
        const uint32_t d = __float_as_uint(L.po.y);
        cp.hit[slot] = make_uint2(d, d == __float_as_uint(tmax) ? NO_TRI : L.triID);
    }
}

// refill_occluder (uvrt_occlude.hip) with this kernel's retire: the lane starts at dist = tmax
template <int FL>
__device__ __forceinline__ void refill_closest(LaneF& L, const ClosestParams& cp, float& tmax, uint32_t& special, uint32_t& slot,
                                               unsigned long long idle_mask, uint32_t cursor, uint32_t wave, uint32_t W,
                                               uint32_t root)
{
    const ExtendParams& p = cp.e;
    retire_closest(L, cp, tmax, slot);
    slot = NO_SLOT;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_mask, 0u));
    const uint32_t v = cursor + rank;
    const uint32_t gb = (v >> 6) * W + wave;                 // global 64-slot batch
    const uint32_t my = gb * 64u + (v & 63u);
    if (v < p.chunk && my < (uint32_t)p.n) {
        const float4 rec = p.rays[my];
        const float2 o = cp.oxz[my];
        const float tm = cp.tmax[my];
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

template <int FL>
__global__ __launch_bounds__(256, FREE_GRID_PER_CU) void k_closest_free(ClosestParams cp)
{
    static_assert(FL == 0 || FL == 1, "closest hits: flavours 0 and 1");
    const ExtendParams& p = cp.e;
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
    float tmax = 1e30f;
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
                if (L.cur == REF_DONE) refill_closest<FL>(L, cp, tmax, special, slot, idle_mask, cursor, wave, W, p.root_ref6);
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
    retire_closest(L, cp, tmax, slot);
}

bool launch_closest_free(const ClosestParams& p0, int grid_per_cu, hipStream_t s)
{
    if (p0.e.n <= 0) return true;
    ClosestParams cp = p0;
    ExtendParams& p = cp.e;
    if (p.flavour != 0 && p.flavour != 1) return false;
    p.order = nullptr;
    p.hits = nullptr;
    p.plane_batches = 0;                    // one launch, one plane
    const unsigned grid = size_persistent_grid(p, grid_per_cu < FREE_GRID_PER_CU ? grid_per_cu : FREE_GRID_PER_CU);
    if (grid == 0) return false;
    p.root_ref6 = (p.scene.root_ref >= REF_LEAF_BIT && p.scene.root_ref != REF_DONE)
                      ? p.scene.root_ref + (uint32_t)p.npairs : p.scene.root_ref;
    if (p.flavour == 1) hipLaunchKernelGGL((k_closest_free<1>), dim3(grid), dim3(256), 0, s, cp);
    else hipLaunchKernelGGL((k_closest_free<0>), dim3(grid), dim3(256), 0, s, cp);
    return true;
}

// ---- the one-bounce gather ----

// n = cross(e1, e2) in f64 and its length (uvrt_occlude.hip's tri_normal: the same expression)
__device__ __forceinline__ double tri_normal2(const float4 e1, const float4 e2, double& nx, double& ny, double& nz)
{
    const double ax = (double)e1.x, ay = (double)e1.y, az = (double)e1.z;
    const double bx = (double)e2.x, by = (double)e2.y, bz = (double)e2.z;
    nx = ay * bz - az * by;
    ny = az * bx - ax * bz;
    nz = ax * by - ay * bx;
    return sqrt(nx * nx + ny * ny + nz * nz);
}

__device__ __forceinline__ bool finite_f32(float v) { return (__float_as_uint(v) & 0x7F800000u) != 0x7F800000u; }

__global__ __launch_bounds__(256) void k_indirect_generate(IndirectGenParams g)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)g.tri_count * g.samples) return;
    const uint32_t lt = (uint32_t)(i / g.samples), s = (uint32_t)(i - (int64_t)lt * g.samples);
    const uint32_t t = (uint32_t)g.first_tri + lt;
    const uint32_t j = t * (uint32_t)g.samples + s;
    uint32_t rng = wang_hash(j ^ g.seed_hash);
    float a = random_float(rng);
    float b = random_float(rng);
    if (a + b > 1.0f) { a = 1.0f - a; b = 1.0f - b; }
    const float4 v0 = g.gtris[(size_t)t * 3 + 0], e1 = g.gtris[(size_t)t * 3 + 1], e2 = g.gtris[(size_t)t * 3 + 2];
    const float px = (v0.x + a * e1.x) + b * e2.x;
    const float py = (v0.y + a * e1.y) + b * e2.y;
    const float pz = (v0.z + a * e1.z) + b * e2.z;
    // generate.cl:25-28's point in the unit disc, bounded: after 8 rejected rounds the centre
    double x = 0.0, y = 0.0;
    for (int round = 0; round < 8; ++round) {
        const float xf = random_float(rng);
        const float yf = random_float(rng);
        const double xd = (double)(xf * 2.0f - 1.0f), yd = (double)(yf * 2.0f - 1.0f);
        if (xd * xd + yd * yd <= 1.0) { x = xd; y = yd; break; }
    }
    double nx, ny, nz;
    const double nn = tri_normal2(e1, e2, nx, ny, nz);
    const double Ex = (double)e1.x, Ey = (double)e1.y, Ez = (double)e1.z;
    const double l1 = sqrt((Ex * Ex + Ey * Ey) + Ez * Ez);
    const double Tx = Ex / l1, Ty = Ey / l1, Tz = Ez / l1;
    const double Bx = (ny * Tz - nz * Ty) / nn, By = (nz * Tx - nx * Tz) / nn, Bz = (nx * Ty - ny * Tx) / nn;
    const double z = sqrt(1.0 - (x * x + y * y));
    const double zz = ((s & 1u) ? -z : z) / nn;
    const float dx = (float)(((x * Tx) + (y * Bx)) + (zz * nx));
    const float dy = (float)(((x * Ty) + (y * By)) + (zz * ny));
    const float dz = (float)(((x * Tz) + (y * Bz)) + (zz * nz));
    float4 ray = make_float4(dx, dy, dz, py);
    float tm = 1e30f;
    if (nn == 0.0 || !finite_f32(dx) || !finite_f32(dy) || !finite_f32(dz) || (dx == 0.0f && dy == 0.0f && dz == 0.0f)) {
        ray = make_float4(0.f, 1.f, 0.f, py);       // not traced: tmax 0 accepts no hit
        tm = 0.0f;
    }
    g.rays[i] = ray;
    g.oxz[i] = make_float2(px, pz);
    g.tmax[i] = tm;
}

void launch_indirect_generate(const IndirectGenParams& p, hipStream_t s)
{
    const int64_t n = (int64_t)p.tri_count * p.samples;
    if (n <= 0) return;
    hipLaunchKernelGGL(k_indirect_generate, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, s, p);
}

__global__ __launch_bounds__(256) void k_indirect_reduce(IndirectReduceParams r)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= r.tri_count) return;
    const size_t t = (size_t)r.first_tri + (size_t)i;
    double nx, ny, nz;
    const double nn = tri_normal2(r.gtris[t * 3 + 1], r.gtris[t * 3 + 2], nx, ny, nz);
    double sum = 0.0;
    const size_t at = (size_t)i * (size_t)r.samples;
    for (int32_t s = 0; s < r.samples; ++s) {
        const uint32_t h = r.hit[at + s].y;
        double ys = 0.0;
        if (h < (uint32_t)r.T && h != (uint32_t)t) {        // (NO_TRI, a miss, is no triangle's id)
            const double nh = tri_normal2(r.gtris[(size_t)h * 3 + 1], r.gtris[(size_t)h * 3 + 2], nx, ny, nz);
            if (nh > 0.0) ys = r.source[h] / (0.5 * nh);
        }
        sum = sum + ys;
    }
    const double ind = nn == 0.0 ? 0.0 : ((double)r.reflectance * (0.5 * nn)) * ((2.0 * sum) / (double)r.samples);
    r.expected[t] = r.add ? r.expected[t] + ind : ind;
}

void launch_indirect_reduce(const IndirectReduceParams& p, hipStream_t s)
{
    if (p.tri_count <= 0) return;
    hipLaunchKernelGGL(k_indirect_reduce, dim3((unsigned)((p.tri_count + 255) / 256)), dim3(256), 0, s, p);
}

// Test hook: the rays of a chunk as the reference's 32-byte Ray records, dist = tmax
__global__ __launch_bounds__(256) void k_export_closest_rays(const float4* __restrict__ rays, const float2* __restrict__ oxz,
                                                             const float* __restrict__ tmax, float4* __restrict__ out, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float4 rec = rays[i];
    const float2 o = oxz[i];
    out[i * 2 + 0] = make_float4(rec.x, rec.y, rec.z, o.x);
    out[i * 2 + 1] = make_float4(rec.w, o.y, tmax[i], 0.f);
}

void launch_export_closest_rays(const float4* rays, const float2* oxz, const float* tmax, void* out32, int64_t count, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_export_closest_rays, dim3((unsigned)((count + 255) / 256)), dim3(256), 0, s, rays, oxz, tmax,
                       (float4*)out32, count);
}

}  // namespace uvrt

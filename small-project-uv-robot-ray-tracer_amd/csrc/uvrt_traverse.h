// uvrt_traverse.h -- device helpers shared by the traversal kernels (uvrt_extend6.hip: the reference's
// BVH2 order for the rays of one lamp column; uvrt_extend_free.hip: the same for rays of any origin;
// uvrt_extend4.hip: the opt-in 4-wide collapse): exact slab distances, box and triangle tests, the
// per-lane ray state, the ray feed (refill, retire, grid sizing), the stack-overflow pointer, and the
// BVH2 traversal step itself (step6 / step7: ONE function each for k_extend6 and k_extend_free).  See
// uvrt_extend6.hip's header for the arithmetic.
#pragma once
#include "uvrt_device.h"

namespace uvrt {

typedef float v2f __attribute__((ext_vector_type(2)));
typedef float v4f __attribute__((ext_vector_type(4)));

constexpr int MAXS6 = 32;                 // extend.cl:43
constexpr int PS6 = 8;                    // LDS stack entries per lane.  7.5 % of the trips of the test room see a deeper
                                          // stack and take the general step (1.6 % with 9 rows, 0.35 % with 10:
                                          // tests/tools/trip_stats.sh), but more rows gain nothing: 9 rows with 123 cached
                                          // records (still eight workgroups per CU) measure the same, 10 rows lose 5 % --
                                          // launch pipelining lives on the eighth workgroup slot of a CU
constexpr uint32_t TOP6_STRIDE = 64;      // bytes per cached record.  (80 with 16 bytes of padding spread the lanes of a
                                          // ds_read_b128 over more banks, but LDS reads cost a trip nothing measurable and 48
                                          // more records do: +2 %, profiles/r02/r02_experiments.txt)

// The six slab distances of one child box (extend.cl:31-37), correctly rounded:
//   t = a / d  as  q0 = a * y;  r = fma(-d, q0, a);  q = fma(r, y, q0),   y = RN32(1/d)
// for the three (min, max) numerator pairs x, z (already a = b - o) and y (raw bounds: the ray's
// origin y is subtracted first).  px/py/pz = {d, y} per axis, po = {origin y, .}; every step is one
// packed instruction with the broadcast of d, y or o done by op_sel.  One asm block so that the
// three chains are interleaved by hand and need exactly three temporary register pairs.
__device__ __forceinline__ void slabs6(v2f& x, v2f& y, v2f& z, v2f px, v2f py, v2f pz, v2f po)
{
    v2f tx, ty, tz;
    asm("v_pk_add_f32 %[y], %[y], %[po] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[tx], %[x], %[px] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %[tz], %[z], %[pz] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %[ty], %[y], %[py] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_fma_f32 %[x], %[px], %[tx], %[x] op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
        "v_pk_fma_f32 %[z], %[pz], %[tz], %[z] op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
        "v_pk_fma_f32 %[y], %[py], %[ty], %[y] op_sel:[0,0,0] op_sel_hi:[0,1,1] neg_lo:[1,0,0] neg_hi:[1,0,0]\n\t"
        "v_pk_fma_f32 %[x], %[x], %[px], %[tx] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[z], %[z], %[pz], %[tz] op_sel:[0,1,0] op_sel_hi:[1,1,1]\n\t"
        "v_pk_fma_f32 %[y], %[y], %[py], %[ty] op_sel:[0,1,0] op_sel_hi:[1,1,1]"
        : [x] "+v"(x), [y] "+v"(y), [z] "+v"(z), [tx] "=&v"(tx), [ty] "=&v"(ty), [tz] "=&v"(tz)
        : [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [po] "v"(po));
}

// The same six distances in the "shipped flags" flavour (uvrt_set_flavour 2): t = (b - o) * v_rcp_f32(d), with the
// reciprocal in the high half of px / py / pz -- what the reference's own build flags make of extend.cl:31-35
__device__ __forceinline__ void slabs6s(v2f& x, v2f& y, v2f& z, v2f px, v2f py, v2f pz, v2f po)
{
    asm("v_pk_add_f32 %[y], %[y], %[po] op_sel_hi:[1,0] neg_lo:[0,1] neg_hi:[0,1]\n\t"
        "v_pk_mul_f32 %[x], %[x], %[px] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %[z], %[z], %[pz] op_sel:[0,1] op_sel_hi:[1,1]\n\t"
        "v_pk_mul_f32 %[y], %[y], %[py] op_sel:[0,1] op_sel_hi:[1,1]"
        : [x] "+v"(x), [y] "+v"(y), [z] "+v"(z)
        : [px] "v"(px), [py] "v"(py), [pz] "v"(pz), [po] "v"(po));
}

// extend.cl:29-38 from the three (t at min, t at max) pairs: entry distance and hit flag.  No operand
// is NaN on this path, so v_min/v_max equal OpenCL's y<x?y:x / x<y?y:x.
__device__ __forceinline__ bool box_fast(v2f tx, v2f ty, v2f tz, float dist, float& tmin)
{
    float nx, fx, ny, fy, nz, fz, tmax;
    asm("v_min_f32 %0, %1, %2" : "=v"(nx) : "v"(tx.x), "v"(tx.y));
    asm("v_max_f32 %0, %1, %2" : "=v"(fx) : "v"(tx.x), "v"(tx.y));
    asm("v_min_f32 %0, %1, %2" : "=v"(ny) : "v"(ty.x), "v"(ty.y));
    asm("v_max_f32 %0, %1, %2" : "=v"(fy) : "v"(ty.x), "v"(ty.y));
    asm("v_min_f32 %0, %1, %2" : "=v"(nz) : "v"(tz.x), "v"(tz.y));
    asm("v_max_f32 %0, %1, %2" : "=v"(fz) : "v"(tz.x), "v"(tz.y));
    asm("v_max3_f32 %0, %1, %2, %3" : "=v"(tmin) : "v"(nx), "v"(ny), "v"(nz));   // max(max(nx, ny), nz)
    asm("v_min3_f32 %0, %1, %2, %3" : "=v"(tmax) : "v"(fx), "v"(fy), "v"(fz));   // min(min(fx, fy), fz)
    return (tmax >= tmin) & (tmin < dist) & (tmax > 0);
}

// extend.cl:29-38 for BOTH child boxes in one block (no hazard padding between statements): entry and exit
// distances from the (t at min, t at max) pairs.  No operand is NaN on this path.
__device__ __forceinline__ void box2_fast(v2f tx0, v2f ty0, v2f tz0, v2f tx1, v2f ty1, v2f tz1, float& tmin0, float& tmax0,
                                          float& tmin1, float& tmax1)
{
    float a, b, c;
    asm("v_min_f32 %[a], %[x0l], %[x0h]\n\t"
        "v_min_f32 %[b], %[y0l], %[y0h]\n\t"
        "v_min_f32 %[c], %[z0l], %[z0h]\n\t"
        "v_max3_f32 %[n0], %[a], %[b], %[c]\n\t"
        "v_max_f32 %[a], %[x0l], %[x0h]\n\t"
        "v_max_f32 %[b], %[y0l], %[y0h]\n\t"
        "v_max_f32 %[c], %[z0l], %[z0h]\n\t"
        "v_min3_f32 %[f0], %[a], %[b], %[c]\n\t"
        "v_min_f32 %[a], %[x1l], %[x1h]\n\t"
        "v_min_f32 %[b], %[y1l], %[y1h]\n\t"
        "v_min_f32 %[c], %[z1l], %[z1h]\n\t"
        "v_max3_f32 %[n1], %[a], %[b], %[c]\n\t"
        "v_max_f32 %[a], %[x1l], %[x1h]\n\t"
        "v_max_f32 %[b], %[y1l], %[y1h]\n\t"
        "v_max_f32 %[c], %[z1l], %[z1h]\n\t"
        "v_min3_f32 %[f1], %[a], %[b], %[c]"
        : [n0] "=&v"(tmin0), [f0] "=&v"(tmax0), [n1] "=&v"(tmin1), [f1] "=&v"(tmax1), [a] "=&v"(a), [b] "=&v"(b), [c] "=&v"(c)
        : [x0l] "v"(tx0.x), [x0h] "v"(tx0.y), [y0l] "v"(ty0.x), [y0h] "v"(ty0.y), [z0l] "v"(tz0.x), [z0h] "v"(tz0.y),
          [x1l] "v"(tx1.x), [x1h] "v"(tx1.y), [y1l] "v"(ty1.x), [y1h] "v"(ty1.y), [z1l] "v"(tz1.x), [z1h] "v"(tz1.y));
}

// the reference's own form: IEEE divisions, OpenCL min/max as selects (NaN operands: 0/0)
__device__ __forceinline__ bool box_exact(float ax1, float ax2, float ay1, float ay2, float az1, float az2,
                                          float dx, float dy, float dz, float dist, float& tmin_out)
{
    const float tx1 = ax1 / dx, tx2 = ax2 / dx;
    float tmin = tx2 < tx1 ? tx2 : tx1, tmax = tx1 < tx2 ? tx2 : tx1;
    const float ty1 = ay1 / dy, ty2 = ay2 / dy;
    const float mny = ty2 < ty1 ? ty2 : ty1, mxy = ty1 < ty2 ? ty2 : ty1;
    tmin = tmin < mny ? mny : tmin;
    tmax = mxy < tmax ? mxy : tmax;
    const float tz1 = az1 / dz, tz2 = az2 / dz;
    const float mnz = tz2 < tz1 ? tz2 : tz1, mxz = tz1 < tz2 ? tz2 : tz1;
    tmin = tmin < mnz ? mnz : tmin;
    tmax = mxz < tmax ? mxz : tmax;
    tmin_out = tmin;
    return tmax >= tmin && tmin < dist && tmax > 0;
}

// RN32(1 / a) for 2^-64 <= |a| < 2^64 (file header)
__device__ __forceinline__ float rcp_exact(float a)
{
    float y0;
    asm("v_rcp_f32 %0, %1" : "=v"(y0) : "v"(a));
    const float e = __builtin_fmaf(-a, y0, 1.0f);
    return __builtin_fmaf(e, y0, y0);
}

// v_rcp_f32 as it is (about 1 ulp): the reciprocal of the "shipped flags" flavour
__device__ __forceinline__ float rcp_raw(float a)
{
    float y;
    asm("v_rcp_f32 %0, %1" : "=v"(y) : "v"(a));
    return y;
}

// extend.cl:6-27 on a leaf record (v0, e1 = v1 - v0, e2 = v2 - v0, id in v0.w).
// FL = the arithmetic flavour (include/uvrt.h uvrt_set_flavour):
//   0  strict: every operator one rounding, source order;
//   1  "ocl-amd": cross() and dot() in the fused forms ROCm's OpenCL device library gives the reference's
//      extend.cl on gfx950 (read off the disassembly of that kernel as built for gfx950):
//      cross(a, b).x = fma(a.y, b.z, -(a.z * b.y)), dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x));
//      everything else as extend.cl writes it;
//   2  "shipped flags": what the reference's OWN build options (-cl-fast-relaxed-math -cl-mad-enable,
//      template/template.cpp:1192) make of extend.cl on gfx950 (read off the disassembly of that build, which the tests run live beside this): the
//      fused forms of flavour 1, f = v_rcp_f32(a) without refinement, and the early returns in the forms the
//      no-NaN licence gives them (|a| >= 1e-5, 0 <= u, 1 >= u, 0 <= v, 1 >= v + u continue).
template <int FL>
__device__ __forceinline__ float cross6(float ay, float bz, float az, float by)
{
    return FL != 0 ? __builtin_fmaf(ay, bz, -(az * by)) : ay * bz - az * by;
}
template <int FL>
__device__ __forceinline__ float dot6(float ax, float ay, float az, float bx, float by, float bz)
{
    return FL != 0 ? __builtin_fmaf(az, bz, __builtin_fmaf(ay, by, ax * bx)) : ax * bx + ay * by + az * bz;
}
template <int FL>
__device__ __forceinline__ void tri6(float ox, float oy, float oz, float dx, float dy, float dz, float& dist,
                                     uint32_t& triID, const float4 v0, const float4 e1, const float4 e2,
                                     bool exact)
{
    const float hx = cross6<FL>(dy, e2.z, dz, e2.y);
    const float hy = cross6<FL>(dz, e2.x, dx, e2.z);
    const float hz = cross6<FL>(dx, e2.y, dy, e2.x);
    const float a = dot6<FL>(e1.x, e1.y, e1.z, hx, hy, hz);
    if (FL == 2 ? !(fabsf(a) >= 0.00001f) : fabsf(a) < 0.00001f) return;
    float f;
    if (FL == 2) f = rcp_raw(a);
    else if (exact) f = 1.0f / a;         // wave-uniform
    else f = rcp_exact(a);
    const float sx = ox - v0.x, sy = oy - v0.y, sz = oz - v0.z;
    const float u = f * dot6<FL>(sx, sy, sz, hx, hy, hz);
    if (FL == 2 ? !((0.0f <= u) & (1.0f >= u)) : ((u < 0) | (u > 1))) return;
    const float qx = cross6<FL>(sy, e1.z, sz, e1.y);
    const float qy = cross6<FL>(sz, e1.x, sx, e1.z);
    const float qz = cross6<FL>(sx, e1.y, sy, e1.x);
    const float v = f * dot6<FL>(dx, dy, dz, qx, qy, qz);
    if (FL == 2 ? !((0.0f <= v) & (1.0f >= u + v)) : ((v < 0) | (u + v > 1))) return;
    const float tt = f * dot6<FL>(e2.x, e2.y, e2.z, qx, qy, qz);
    if (tt > 0.0001f && tt < dist) {
        dist = tt;
        triID = __float_as_uint(v0.w);
    }
}

// extend.cl:29-38 in the "shipped flags" flavour: t = (b - o) * v_rcp_f32(d) (the numerators arrive as b - o, the
// reciprocals in the ray's {d, rcp} pairs), then the same hardware min / max as box_fast
__device__ __forceinline__ bool box_shipped(float ax1, float ax2, float ay1, float ay2, float az1, float az2,
                                            float rx, float ry, float rz, float dist, float& tmin)
{
    const v2f tx = {ax1 * rx, ax2 * rx}, ty = {ay1 * ry, ay2 * ry}, tz = {az1 * rz, az2 * rz};
    return box_fast(tx, ty, tz, dist, tmin);
}

// In-place update of a loop-carried value inside a divergent branch: the write happens under the
// branch's exec mask into the SAME register, so hipcc has no second copy of the value to merge (it
// otherwise keeps a loop-carried and an in-body copy of the ray constants and moves one into the
// other on every trip).
__device__ __forceinline__ void set_in_place(float& dst, float v) { asm volatile("v_mov_b32 %0, %1" : "+v"(dst) : "v"(v)); }
__device__ __forceinline__ void set_in_place(uint32_t& dst, uint32_t v) { asm volatile("v_mov_b32 %0, %1" : "+v"(dst) : "v"(v)); }
__device__ __forceinline__ void set_in_place(int& dst, int v) { asm volatile("v_mov_b32 %0, %1" : "+v"(dst) : "v"(v)); }
__device__ __forceinline__ void set_in_place(v2f& dst, float lo, float hi)
{
    const v2f v = {lo, hi};
    asm volatile("v_pk_mov_b32 %0, %1, %1 op_sel:[0,1]" : "+v"(dst) : "v"(v));
}

struct Lane6 {
    static constexpr bool OWN_XZ = false;   // x / z of the origin are the launch's (p.ox, p.oz); the records hold b - o
    v2f px, py, pz;         // {d, RN32(1/d)} per axis
    v2f po;                 // {origin y, dist}
    uint32_t triID;
    uint32_t cur;           // record reference: index | leaf bit + count code, REF_DONE = no ray
    int sp;
};

// the lane of a ray that carries its own origin (k_extend_free): the records hold the raw bounds, a step forms b - o
struct LaneF : Lane6 {
    static constexpr bool OWN_XZ = true;
    v2f oxz;                // {origin x, origin z}
};

// x / z of the origin of a lane's ray, for the triangle test (asked for where it is used: a copy made at the top of a step
// changes the order of hipcc's instructions)
__device__ __forceinline__ float origin_x(const Lane6&, const ExtendParams& p) { return p.ox; }
__device__ __forceinline__ float origin_z(const Lane6&, const ExtendParams& p) { return p.oz; }
__device__ __forceinline__ float origin_x(const LaneF& L, const ExtendParams&) { return L.oxz.x; }
__device__ __forceinline__ float origin_z(const LaneF& L, const ExtendParams&) { return L.oxz.y; }

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

// ---- the persistent ray feed of k_extend6, k_extend4 and k_extend_free ----
// ints from a wave's replica of the counts to the plane of a lane's ray (the kernels' plane_off; bit 31 of that register:
// the ray needs the exact step)
constexpr uint32_t PLANE_OFF6 = 0x7FFFFFFFu, SPECIAL6 = 0x80000000u;

// A ray outside the proof conditions of the packed exact division (a direction component zero, NaN, > 1 or
// < 2^-60; an origin height that is tiny but not zero, or huge): it runs the IEEE-division form of the step.
// Range tests on the bit patterns: |x| in [lo, hi]  <=>  bits(|x|) - bits(lo) <= bits(hi) - bits(lo) as unsigned.
__device__ __forceinline__ bool outside_proof_conditions(float4 rec)
{
    const uint32_t lo = 0x21800000u /* 2^-60 */, one = 0x3F800000u;
    const uint32_t ux = (__float_as_uint(rec.x) & 0x7FFFFFFFu) - lo, uy = (__float_as_uint(rec.y) & 0x7FFFFFFFu) - lo,
                   uz = (__float_as_uint(rec.z) & 0x7FFFFFFFu) - lo;
    const uint32_t worst = max(max(ux, uy), uz);
    const uint32_t uo = __float_as_uint(rec.w) & 0x7FFFFFFFu;                   // |origin y|
    const uint32_t ylo = 0x0D800000u /* 2^-100 = 7.888609e-31f */, yhi = 0x4E6E6B28u /* 1e9f */;
    return worst > one - lo || (uo != 0u && uo - ylo > yhi - ylo);
}

// |o| zero or in [2^-100, 1e9]: the window outside_proof_conditions applies to the origin's y
__device__ __forceinline__ bool origin_outside_window(float o)
{
    const uint32_t uo = __float_as_uint(o) & 0x7FFFFFFFu;
    const uint32_t lo = 0x0D800000u /* 2^-100 */, hi = 0x4E6E6B28u /* 1e9f */;
    return uo != 0u && uo - lo > hi - lo;
}

// The results of the ray a lane has finished (extend.cl:94-98): its hit record when one is pending (`live`), and its deposit
// unless it hit nothing (dist == 1e30f).
// DD: the ray of a deduped chunk (uvrt_dedupe.h) -- the register holds the ray's deposit word instead of one plane's offset:
// a plane index (the launch's own plane, or the class plane of its mask: one deposit at index * plane_stride + triID), or the
// MASK of its planes, deposited once per set bit at bit * plane_stride + triID (uint32: a batch has fewer than 2^32 counters).
template <bool RECORD, bool DD = false>
__device__ __forceinline__ void retire_ray(const Lane6& L, const ExtendParams& p, int32_t* my_counts, uint32_t plane_off,
                                           uint32_t slot, bool live, uint32_t cls_delta = 0u)
{
    if (RECORD && live && p.hits) {
        const uint32_t li = p.order ? p.order[slot] : slot;
        p.hits[li] = make_uint2(__float_as_uint(L.po.y), L.triID);
    }
    if constexpr (DD) {
        if (L.po.y != 1e30f) {
            const uint32_t w = plane_off & PLANE_OFF6;
            // (a chunk without classes holds masks only, and bit 30 may be a launch there: p.cls_replicas == 0)
            if (w & (p.cls_replicas != 0 ? uvrt::DEDUPE_PLANE_FORM : 0u))      // one plane: the launch's own, or the class plane of the ray's mask
                atomicAdd(&my_counts[(w & uvrt::DEDUPE_PLANE_INDEX) * p.plane_stride + L.triID + ((w & uvrt::DEDUPE_CLASS_FORM) ? cls_delta : 0u)], 1);
            else
                for (uint32_t m = w; m != 0u; m &= m - 1u)
                    atomicAdd(&my_counts[(uint32_t)__builtin_ctz(m) * p.plane_stride + L.triID], 1);
        }
    } else
    if (L.po.y != 1e30f) atomicAdd(&my_counts[(plane_off & PLANE_OFF6) + L.triID], 1);
}

// Does a launch hold the planes of a batch (include/uvrt.h uvrt_trace_batch_launches)?  k_extend6 / k_extend4 ask the launch
// (p.plane_stride != 0: one kernel serves both); k_extend_free is compiled for either answer.
enum PlaneMode { PLANES_ASK, PLANES_NONE, PLANES_ALL };

// The per-lane part of a refill, for an idle lane (L.cur == REF_DONE): retire its last ray, then take slot cursor + (rank among
// the idle lanes) of the wave's sequence of 64-ray batches wave, wave + W, wave + 2W, ...  A slot beyond the wave's share, the
// launch or its plane leaves the lane idle.  `root`: the kernel's root reference; `oxz`: the rays' {origin x, origin z}, read for
// a lane that carries them (LaneF).
// DD: a deduped chunk (uvrt_dedupe.h) -- one compacted list of dd_n rays (read from device memory by the kernel's prologue, as is
// the wave's share dd_chunk), no planes in it: the ray's mask is loaded beside the ray, behind the same wait, and takes the
// place of the plane offset (bit 31 is the exact-step flag either way).
template <bool RECORD, int FL, PlaneMode PM = PLANES_ASK, bool DD = false, class LaneT>
__device__ __forceinline__ void refill_lane(LaneT& L, const ExtendParams& p, const float2* oxz, int32_t* my_counts,
                                            uint32_t& plane_off, uint32_t& slot, bool& live, unsigned long long idle_mask,
                                            uint32_t cursor, uint32_t wave, uint32_t W, uint32_t root,
                                            uint32_t dd_chunk = 0u, uint32_t dd_n = 0u, uint32_t cls_delta = 0u)
{
    retire_ray<RECORD, DD>(L, p, my_counts, plane_off, slot, live, cls_delta);
    live = false;
    L.po.y = 1e30f;
    const uint32_t rank = __builtin_amdgcn_mbcnt_hi((uint32_t)(idle_mask >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)idle_mask, 0u));
    const uint32_t v = cursor + rank;
    const uint32_t gb = (v >> 6) * W + wave;                 // global 64-slot batch
    const uint32_t my = gb * 64u + (v & 63u);
    if constexpr (DD) {
        static_assert(!LaneT::OWN_XZ && !RECORD, "deduped chunks are k_extend6's, and a batch records no hits");
        if (v < dd_chunk && my < dd_n) {
            const float4 rec = p.rays[my];
            const uint32_t mask = p.masks[my];
            set_in_place(L.px, rec.x, FL == 2 ? rcp_raw(rec.x) : rcp_exact(rec.x));
            set_in_place(L.py, rec.y, FL == 2 ? rcp_raw(rec.y) : rcp_exact(rec.y));
            set_in_place(L.pz, rec.z, FL == 2 ? rcp_raw(rec.z) : rcp_exact(rec.z));
            set_in_place(L.po, rec.w, 1e30f);       // generate.cl:34-35
            set_in_place(L.triID, 0u);
            set_in_place(L.sp, 0);
            set_in_place(L.cur, root);
            const bool spec = FL != 2 && (outside_proof_conditions(rec) || p.force_exact != 0);
            set_in_place(plane_off, mask | (spec ? SPECIAL6 : 0u));
        }
        return;
    }
    // plane (= launch of a batched trace) of the batch: gb / plane_batches, exact after one
    // correction step (gb < 2^24 is exact in f32, the rounded reciprocal is off by < 1)
    uint32_t pl = 0;
    int32_t within = (int32_t)gb;
    if (PM == PLANES_ASK ? p.plane_stride != 0 : PM == PLANES_ALL) {        // wave-uniform: a launch of its own is one plane
        pl = (uint32_t)((float)gb * p.plane_inv);
        within = (int32_t)(gb - pl * p.plane_batches);
        if (within < 0) { --pl; within += (int32_t)p.plane_batches; }
        else if ((uint32_t)within >= p.plane_batches) { ++pl; within -= (int32_t)p.plane_batches; }
    }
    // The slot is a ray of its plane, not the plane's padding.  A kernel compiled for its answer has that settled before the
    // other two tests; a kernel that asks the launch tests it last.  (The place decides the order of hipcc's instructions.)
    const auto in_plane = [&] { return (uint32_t)within * 64u + (v & 63u) < p.plane_n; };
    const bool settled = PM == PLANES_NONE || (PM == PLANES_ALL && in_plane());
    if (v < p.chunk && my < (uint32_t)p.n && (PM == PLANES_ASK ? in_plane() : settled)) {
        const float4 rec = p.rays[my];
        float2 o = make_float2(0.f, 0.f);
        if constexpr (LaneT::OWN_XZ) o = oxz[my];
        // y = RN32(1/d) (rcp_exact: exact for 2^-64 <= |d| < 2^64; other lanes are `spec`
        // and never use y); flavour 2: y = v_rcp_f32(d), used by every lane
        set_in_place(L.px, rec.x, FL == 2 ? rcp_raw(rec.x) : rcp_exact(rec.x));
        set_in_place(L.py, rec.y, FL == 2 ? rcp_raw(rec.y) : rcp_exact(rec.y));
        set_in_place(L.pz, rec.z, FL == 2 ? rcp_raw(rec.z) : rcp_exact(rec.z));
        set_in_place(L.po, rec.w, 1e30f);       // generate.cl:34-35
        if constexpr (LaneT::OWN_XZ) set_in_place(L.oxz, o.x, o.y);
        set_in_place(L.triID, 0u);
        if (RECORD) { slot = my; live = true; }
        set_in_place(L.sp, 0);
        set_in_place(L.cur, root);
        // (an own x / z origin outside the window of the origin's y: uvrt_extend_free.hip's header)
        bool outside = outside_proof_conditions(rec);
        if constexpr (LaneT::OWN_XZ) outside = outside || origin_outside_window(o.x) || origin_outside_window(o.y);
        const bool spec = FL != 2 && (outside || p.force_exact != 0);
        set_in_place(plane_off, pl * p.plane_stride | (spec ? SPECIAL6 : 0u));
    }
}

// Persistent grid of a traversal launch (launch_extend6, launch_extend4): a single plane of all n rays unless the caller
// batches planes, the refill threshold clamped to 1..64, at most grid_per_cu workgroups per CU and none beyond 256 rays
// each, every wave's share `chunk` in whole 64-ray batches.  Returns the grid, or 0 when its overflow stacks would not fit.
inline unsigned size_persistent_grid(ExtendParams& p, int grid_per_cu)
{
    const unsigned cus = p.num_cus > 0 ? (unsigned)p.num_cus : 256u;
    unsigned grid = cus * (unsigned)grid_per_cu;
    if (p.plane_batches == 0) {      // one launch: a single plane that holds all n rays
        p.plane_batches = (uint32_t)((p.n + 63) / 64);
        p.plane_n = (uint32_t)p.n;
        p.plane_stride = 0;
    }
    p.plane_inv = 1.0f / (float)p.plane_batches;
    p.refill_min = p.refill_min < 1 ? 1 : (p.refill_min > 64 ? 64 : p.refill_min);
    const unsigned need = (unsigned)((p.n + 255) / 256);
    if (need < grid) grid = need;
    const uint64_t waves = (uint64_t)grid * 4;
    p.chunk = (uint32_t)((((uint64_t)p.n + waves - 1) / waves + 63) / 64 * 64);
    return (uint64_t)grid * 256 * (MAXS6 - PS6) > p.ovf_capacity ? 0u : grid;
}

// Stack entries 8..31 of this thread live in global memory (0.02 % of pushes on the test room).  The
// pointer is rebuilt from scratch where it is needed -- opaque to the compiler, which would otherwise
// keep it in two VGPRs (or a scratch slot) across the whole loop.
__device__ __forceinline__ uint32_t* ovf_ptr(const ExtendParams& p)
{
    uint32_t lane, wv;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    asm volatile("s_mov_b32 %0, %1" : "=s"(wv) : "s"(__builtin_amdgcn_readfirstlane(threadIdx.x >> 6)));
    return p.ovf_stack + ((size_t)blockIdx.x * 256 + wv * 64 + lane) * (MAXS6 - PS6);
}

// the lane's number, computed where it is asked for (threadIdx.x, or a mbcnt the compiler can share, would stay live in a vector
// register from the kernel's entry on -- k_extend6 has none to spare)
__device__ __forceinline__ uint32_t lane_now()
{
    uint32_t lane;
    asm volatile("v_mbcnt_lo_u32_b32 %0, -1, 0\n\tv_mbcnt_hi_u32_b32 %0, -1, %0" : "=v"(lane));
    return lane;
}

// the lane's rank among the lanes that are executing (asked for inside a divergent region: no mask to carry there)
__device__ __forceinline__ uint32_t lane_rank_in_exec()
{
    uint32_t r;
    asm volatile("v_mbcnt_lo_u32_b32 %0, exec_lo, 0\n\tv_mbcnt_hi_u32_b32 %0, exec_hi, %0" : "=v"(r));
    return r;
}

// The same for a ray that may have moved to another lane of its workgroup (k_extend6's drain merge): the rows belong to the lane whose
// LDS stack the ray uses.  stack_base = LDS address of that lane's entry -1; the stack array is aligned to its 1 KB rows.
__device__ __forceinline__ uint32_t* ovf_ptr(const ExtendParams& p, uint32_t stack_base)
{
    return p.ovf_stack + ((size_t)blockIdx.x * 256 + ((stack_base >> 2) & 255u)) * (MAXS6 - PS6);
}

// ---- the BVH2 traversal step of k_extend6 (Lane6) and k_extend_free (LaneF) ----
// One traversal step of one lane (extend.cl:44-80): an inner node (both children tested, ordered,
// descend / push / pop) or -- on a leaf trip -- a leaf (its triangles, pop).
// The general step: any mix of lanes, stacks beyond LDS, and -- `exact`, wave-uniform -- the IEEE-division form of the box and
// triangle arithmetic; the record fetch and the descend / push / pop logic are common to both forms.
// A lane with its own x / z origin forms the x / z numerators b - o per ray, as every lane does for y (the same single f32
// subtraction as extend.cl:31,35), and hands that origin to the triangle test.
template <bool TOP, int FL, class LaneT>
__device__ __forceinline__ void step6(LaneT& L, const ExtendParams& p, uint32_t stack_base,
                                      const float4* s_top, uint32_t top_pairs, bool leaf_trip, bool exact,
                                      unsigned long long m_act /* lanes holding a ray */)
{
    const uint32_t cur = L.cur;
    const bool is_inner = cur < REF_LEAF_BIT;
    const bool is_leaf = (cur >= REF_LEAF_BIT) & (cur != REF_DONE) & leaf_trip;
    const uint32_t idx = cur & REF_FIRST_MASK;          // record index (inner indices are < 2^27 too)
    // ONE asm block fetches the 64-byte record of every stepping lane -- from the LDS top-of-tree
    // cache or from global memory, chosen by exec masks -- and the lane's stack top, so that both
    // sources write the same registers (hipcc otherwise merges the two branches with v_mov chains).
    v4f w0, w1, w2, w3;
    uint32_t spec_top = REF_DONE;                       // stays REF_DONE when the stack is empty
    // stack entry sp - 1 of this lane (lanes with sp == 0 are masked off); entry sp is 1024 bytes on
    const uint32_t sa = stack_base + ((uint32_t)L.sp << 10);
    {
        // lane masks from single comparisons, combined as 64-bit integers (SALU): a ballot of a
        // compound condition would go through a v_cndmask / v_cmp pair
        const unsigned long long m_in = __builtin_amdgcn_ballot_w64(cur < REF_LEAF_BIT);
        const unsigned long long m_top = TOP ? __builtin_amdgcn_ballot_w64(cur < top_pairs) : 0ull;
        const unsigned long long m_sp = __builtin_amdgcn_ballot_w64(L.sp > 0);
        const unsigned long long m_go = m_in | (leaf_trip ? (m_act & ~m_in) : 0ull);
        const unsigned long long m_glob = m_go & ~m_top;
        const unsigned long long m_stk = m_go & m_sp;
        // LDS copy of record r at byte TOP6_STRIDE * r
        const uint32_t a0 = (uint32_t)(uintptr_t)s_top + cur * TOP6_STRIDE;
        // byte offset of the record: the shift drops the leaf flag and count bits of a reference
        // (record indices are < 2^26: uvrt_capi.hip checks P + T), the base address is scalar
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
        // the x / z numerators of the forms that take scalars: the record's value (already b - o), or b - the lane's own origin
        const auto ax = [&](float b) { return LaneT::OWN_XZ ? b - origin_x(L, p) : b; };
        const auto az = [&](float b) { return LaneT::OWN_XZ ? b - origin_z(L, p) : b; };
        if (FL == 2) {        // "shipped flags": t = (b - o) * v_rcp_f32(d) for every lane (there is no other form of it)
            h0 = box_shipped(ax(w0.x), ax(w0.y), w2.x - L.po.x, w2.y - L.po.x, az(w0.z), az(w0.w), L.px.y, L.py.y, L.pz.y, L.po.y, d0);
            h1 = box_shipped(ax(w1.x), ax(w1.y), w2.z - L.po.x, w2.w - L.po.x, az(w1.z), az(w1.w), L.px.y, L.py.y, L.pz.y, L.po.y, d1);
        } else if (exact) {
            h0 = box_exact(ax(w0.x), ax(w0.y), w2.x - L.po.x, w2.y - L.po.x, az(w0.z), az(w0.w), L.px.x, L.py.x, L.pz.x, L.po.y, d0);
            h1 = box_exact(ax(w1.x), ax(w1.y), w2.z - L.po.x, w2.w - L.po.x, az(w1.z), az(w1.w), L.px.x, L.py.x, L.pz.x, L.po.y, d1);
        } else {
            v2f x0 = __builtin_shufflevector(w0, w0, 0, 1), z0 = __builtin_shufflevector(w0, w0, 2, 3);
            v2f x1 = __builtin_shufflevector(w1, w1, 0, 1), z1 = __builtin_shufflevector(w1, w1, 2, 3);
            v2f y0 = __builtin_shufflevector(w2, w2, 0, 1), y1 = __builtin_shufflevector(w2, w2, 2, 3);
            if constexpr (LaneT::OWN_XZ) sub_xz(x0, z0, x1, z1, L.oxz);
            slabs6(x0, y0, z0, L.px, L.py, L.pz, L.po);
            h0 = box_fast(x0, y0, z0, L.po.y, d0);
            slabs6(x1, y1, z1, L.px, L.py, L.pz, L.po);
            h1 = box_fast(x1, y1, z1, L.po.y, d1);
        }
        // extend.cl:56-76 with dist = 1e30f for a missed child: nearer first, farther pushed
        // dist1 > dist2 of extend.cl:61 with 1e30f standing for a miss: child 1 first iff it is hit and
        // child 0 is missed or farther (a hit distance is < dist <= 1e30f, so the sentinel never ties)
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
    // extend.cl:48-55 -- AFTER the inner-node block (other lanes): the triangles of a leaf with several of them
    // are fetched when the node records' registers are free again
    if (is_leaf) {
        uint32_t count = (cur >> REF_COUNT_SHIFT) & 15u;
        const uint32_t first = idx - (uint32_t)p.npairs;
        if (count == 15u) count = p.scene.leaf_count[first];
        float dist = L.po.y;
        tri6<FL>(origin_x(L, p), L.po.x, origin_z(L, p), L.px.x, L.py.x, L.pz.x, dist, L.triID,
             make_float4(w0.x, w0.y, w0.z, w0.w), make_float4(w1.x, w1.y, w1.z, w1.w),
             make_float4(w2.x, w2.y, w2.z, w2.w), exact);
        for (uint32_t i = 1; i < count; ++i) {
            const float4* lt = (const float4*)p.recs + ((size_t)idx + i) * 4;
            tri6<FL>(origin_x(L, p), L.po.x, origin_z(L, p), L.px.x, L.py.x, L.pz.x, dist, L.triID, lt[0], lt[1], lt[2], exact);
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

// The same step for the common case -- no lane needs the IEEE-division form, no lane's stack has left LDS -- with
// the control flow written as lane masks instead of divergent branches.  Scalar issue is the dearest resource of
// this kernel (one instruction per cycle per CU, shared by 32 waves: 32 extra scalar instructions per trip cost
// 17 % of the launch, profiles/r02/r02_experiments.txt), and hipcc spends ~70 of them per trip on exec bookkeeping
// for `if (inner) {...} if (both hit) {push} if (none hit) {pop}`.  Here the caller hands over the lane masks of
// the trip (one vector comparison each), the box arithmetic runs for ALL lanes (a vector instruction costs the
// same whatever its exec mask; lanes that do not stand at an inner node compute on stale registers and are
// masked out of the results), the hit tests narrow exec themselves (v_cmpx), and descend / push / pop are
// exec-masked instructions of one asm block.
//   m_in: lanes at an inner node, m_leaf: lanes that visit their leaf in this trip, m_top: lanes whose record is
//   in the LDS cache, full: the exec mask of the loop (all 64 lanes), clk: takes the cycles of the trip's three parts in a
//   build that asks where they go (k_extend6's TripClock under UVRT_TRIP_STATS); by default there is none.  (`if constexpr`,
//   not an empty member function: a call that is inlined away later still changes the order of hipcc's instructions)
struct NoClock {
    static constexpr bool RUNS = false;
};
template <bool TOP, int FL, class LaneT, class ClockT = NoClock>
__device__ __forceinline__ void step7(LaneT& L, const ExtendParams& p, uint32_t stack_base, uint32_t top_base,
                                      unsigned long long m_in, unsigned long long m_leaf, unsigned long long m_top,
                                      unsigned long long full, ClockT clk = ClockT())
{
    const uint32_t cur = L.cur;
    v4f w0, w1, w2, w3;
    uint32_t spec_top;
    if constexpr (ClockT::RUNS) clk.start();
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
    if constexpr (ClockT::RUNS) clk.lap(0);
    if (m_leaf != 0) {                                       // wave-uniform; m_leaf != 0 means: a leaf trip
        if ((int32_t)cur < -1) {                             // at a leaf (REF_DONE is -1): extend.cl:48-55
            const uint32_t idx = cur & REF_FIRST_MASK;
            uint32_t count = (cur >> REF_COUNT_SHIFT) & 15u;
            const uint32_t first = idx - (uint32_t)p.npairs;
            if (count == 15u) count = p.scene.leaf_count[first];
            float dist = L.po.y;
            tri6<FL>(origin_x(L, p), L.po.x, origin_z(L, p), L.px.x, L.py.x, L.pz.x, dist, L.triID,
                      make_float4(w0.x, w0.y, w0.z, w0.w), make_float4(w1.x, w1.y, w1.z, w1.w),
                      make_float4(w2.x, w2.y, w2.z, w2.w), false);
            for (uint32_t i = 1; i < count; ++i) {
                const float4* lt = (const float4*)p.recs + ((size_t)idx + i) * 4;
                tri6<FL>(origin_x(L, p), L.po.x, origin_z(L, p), L.px.x, L.py.x, L.pz.x, dist, L.triID, lt[0], lt[1], lt[2], false);
            }
            L.po.y = dist;
        }
    }
    if constexpr (ClockT::RUNS) clk.lap(1);
    if (m_in != 0) {            // wave-uniform: a trip with no lane at an inner node skips the box arithmetic
        v2f x0 = __builtin_shufflevector(w0, w0, 0, 1), z0 = __builtin_shufflevector(w0, w0, 2, 3);
        v2f x1 = __builtin_shufflevector(w1, w1, 0, 1), z1 = __builtin_shufflevector(w1, w1, 2, 3);
        v2f y0 = __builtin_shufflevector(w2, w2, 0, 1), y1 = __builtin_shufflevector(w2, w2, 2, 3);
        if constexpr (LaneT::OWN_XZ) sub_xz(x0, z0, x1, z1, L.oxz);
        if (FL == 2) {
            slabs6s(x0, y0, z0, L.px, L.py, L.pz, L.po);
            slabs6s(x1, y1, z1, L.px, L.py, L.pz, L.po);
        } else {
            slabs6(x0, y0, z0, L.px, L.py, L.pz, L.po);
            slabs6(x1, y1, z1, L.px, L.py, L.pz, L.po);
        }
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
    if constexpr (ClockT::RUNS) clk.lap(2);
}

}  // namespace uvrt

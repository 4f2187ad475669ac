// uvrt_refine.hip -- the adaptive gather (include/uvrt.h "adaptive gather"): extra shadow rays for the
// triangles whose first-pass estimate is the least certain.
//
// uvrt_gather_refine works on the planes a uvrt_gather_direct with the variance on has left.  k_refine_count turns
// (expected[t], variance[t]) into n_t, the number of extra samples of triangle t; an exclusive prefix sum over the range
// (k_refine_block_sums, k_refine_scan_sums, k_refine_offsets) gives every triangle's first ray; the host reads the offsets
// once and cuts the range into chunks of at most `capacity` rays.  Per chunk k_refine_generate<MODE> makes the rays -- one
// thread per ray, its triangle found by a search in the offsets, then k_gather_generate's rule with S := n_t --,
// k_occlude_free (uvrt_occlude.hip) answers them and k_refine_reduce<MODE> forms X1, V1 of every refined triangle as
// k_gather_reduce_var<MODE> would at S = n_t and merges them into the planes.  No atomics and sums in sample order: the planes
// are a pure function of what they held and the arguments.
//
// The generate and reduce rules follow k_gather_generate and k_gather_reduce_var (uvrt_occlude.hip) with S := n_t and a merge at
// the end; the triangle normal is the shared tri_normal (uvrt_device.h).  This file is built without contraction, every operator
// below is one rounding.
#include "uvrt_device.h"

namespace uvrt {

constexpr int SCAN_PER_THREAD = 4;
constexpr int SCAN_PER_BLOCK = 256 * SCAN_PER_THREAD;

// The count rule (include/uvrt.h): how many extra samples bring sqrt(variance) / expected down to rel_error, if the extra
// samples scatter like the first S0 did; a power of two in [2, max_extra], or 0.
__global__ __launch_bounds__(256) void k_refine_count(const float4* __restrict__ gtris, const double* __restrict__ expected,
                                                      const double* __restrict__ variance, int32_t* __restrict__ extra, int32_t T,
                                                      int32_t first_tri, int32_t tri_count, int32_t samples0, double rel_error,
                                                      double min_expected, int32_t max_extra)
{
    const int t = blockIdx.x * 256 + threadIdx.x;
    if (t >= T) return;
    int32_t n = 0;
    if (t >= first_tri && t - first_tri < tri_count) {
        double nx, ny, nz;
        const double nn = tri_normal(gtris[(size_t)t * 3 + 1], gtris[(size_t)t * 3 + 2], nx, ny, nz);
        const double X0 = expected[t], V0 = variance[t];
        if (!(nn == 0.0) && X0 > 0.0 && V0 > 0.0 && !(X0 < min_expected)) {
            const double r = rel_error * X0;
            const double want = ceil((double)samples0 * (V0 / (r * r) - 1.0));
            if (!(want >= 1.0)) n = 0;                      // NaN included
            else if (want >= (double)max_extra) n = max_extra;
            else {
                const uint32_t w = (uint32_t)want < 2u ? 2u : (uint32_t)want;       // 2 <= w < max_extra <= 4096
                n = (int32_t)(1u << (32 - __clz((int)(w - 1u))));                   // the smallest power of two >= w
            }
        }
    }
    extra[t] = n;
}

void launch_refine_count(const float4* gtris, const double* expected, const double* variance, int32_t* extra, int32_t T,
                         int32_t first_tri, int32_t tri_count, int32_t samples0, double rel_error, double min_expected,
                         int32_t max_extra, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_refine_count, dim3((unsigned)((T + 255) / 256)), dim3(256), 0, s, gtris, expected, variance, extra, T,
                       first_tri, tri_count, samples0, rel_error, min_expected, max_extra);
}

// ---- the exclusive prefix sum over a range of the n_t plane: integers, so any order of the additions is exact ----

// item i of the scanned sequence: the range's n_t, and one 0 behind them so that position tri_count receives the total
__device__ __forceinline__ int32_t scan_item(const int32_t* __restrict__ extra, int32_t first_tri, int32_t tri_count, int64_t i)
{
    return i < (int64_t)tri_count ? extra[(size_t)first_tri + (size_t)i] : 0;
}

// the sum of the four items of every thread of the block, as an inclusive scan over the threads (`mine` is the thread's own)
__device__ __forceinline__ int32_t scan_block(int32_t mine, int32_t* sh)
{
    sh[threadIdx.x] = mine;
    __syncthreads();
    for (int d = 1; d < 256; d <<= 1) {
        const int32_t below = (int)threadIdx.x >= d ? sh[threadIdx.x - d] : 0;
        __syncthreads();
        sh[threadIdx.x] += below;
        __syncthreads();
    }
    return sh[threadIdx.x];
}

__global__ __launch_bounds__(256) void k_refine_block_sums(const int32_t* __restrict__ extra, int32_t* __restrict__ block_sums,
                                                           int32_t first_tri, int32_t tri_count)
{
    __shared__ int32_t sh[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_BLOCK + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    int32_t mine = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) mine += scan_item(extra, first_tri, tri_count, base + k);
    const int32_t incl = scan_block(mine, sh);
    if (threadIdx.x == 255) block_sums[blockIdx.x] = incl;
}

// one workgroup: block_sums[0, nblocks) becomes its own exclusive prefix sum, tile by tile with a carry
__global__ __launch_bounds__(256) void k_refine_scan_sums(int32_t* __restrict__ block_sums, int32_t nblocks)
{
    __shared__ int32_t sh[256];
    int32_t carry = 0;
    for (int32_t tile = 0; tile < nblocks; tile += 256) {
        const int32_t i = tile + (int32_t)threadIdx.x;
        const int32_t mine = i < nblocks ? block_sums[i] : 0;
        const int32_t incl = scan_block(mine, sh);
        if (i < nblocks) block_sums[i] = carry + (incl - mine);
        carry += sh[255];
        __syncthreads();            // sh[255] is read by every thread before the next tile overwrites it
    }
}

__global__ __launch_bounds__(256) void k_refine_offsets(const int32_t* __restrict__ extra, const int32_t* __restrict__ block_sums,
                                                        int32_t* __restrict__ offs, int32_t first_tri, int32_t tri_count)
{
    __shared__ int32_t sh[256];
    const int64_t base = (int64_t)blockIdx.x * SCAN_PER_BLOCK + (int64_t)threadIdx.x * SCAN_PER_THREAD;
    int32_t item[SCAN_PER_THREAD];
    int32_t mine = 0;
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        item[k] = scan_item(extra, first_tri, tri_count, base + k);
        mine += item[k];
    }
    int32_t run = block_sums[blockIdx.x] + (scan_block(mine, sh) - mine);
    for (int k = 0; k < SCAN_PER_THREAD; ++k) {
        if (base + k <= (int64_t)tri_count) offs[base + k] = run;
        run += item[k];
    }
}

void launch_refine_scan(const int32_t* extra, int32_t* offs, int32_t* block_sums, int32_t first_tri, int32_t tri_count,
                        hipStream_t s)
{
    if (tri_count < 0) return;
    const int32_t nblocks = (int32_t)(((int64_t)tri_count + 1 + SCAN_PER_BLOCK - 1) / SCAN_PER_BLOCK);     // tri_count + 1 positions
    hipLaunchKernelGGL(k_refine_block_sums, dim3((unsigned)nblocks), dim3(256), 0, s, extra, block_sums, first_tri, tri_count);
    hipLaunchKernelGGL(k_refine_scan_sums, dim3(1), dim3(256), 0, s, block_sums, nblocks);
    hipLaunchKernelGGL(k_refine_offsets, dim3((unsigned)nblocks), dim3(256), 0, s, extra, (const int32_t*)block_sums, offs, first_tri,
                       tri_count);
}

// ---- the extra samples ----

// k_gather_generate<MODE> (uvrt_occlude.hip) with a sample count of the triangle's own: ray r of the chunk belongs to the
// triangle whose offsets enclose r + offs[lo], and is its sample s = r + offs[lo] - offs[i] of n_t = offs[i + 1] - offs[i].
template <int MODE>
__global__ __launch_bounds__(256) void k_refine_generate(GatherGenParams g, const int32_t* __restrict__ offs, int32_t lo, int32_t hi,
                                                         int32_t rays)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= (int64_t)rays) return;
    const int32_t at = offs[lo] + (int32_t)i;
    // the last triangle of [lo, hi) whose offset is <= at: offs[lo] <= at < offs[hi], and a triangle without samples shares
    // its offset with its successor, so the one found has n_t > 0
    int32_t a = lo, b = hi;
    while (b - a > 1) {
        const int32_t mid = a + ((b - a) >> 1);
        if (offs[mid] <= at) a = mid; else b = mid;
    }
    const uint32_t samples = (uint32_t)(offs[a + 1] - offs[a]);
    const uint32_t s = (uint32_t)(at - offs[a]);
    const uint32_t t = (uint32_t)g.first_tri + (uint32_t)a;
    const uint32_t j = t * samples + s;
    uint32_t rng = wang_hash(j ^ g.seed_hash);
    float u_h = random_float(rng);
    float u_m = random_float(rng);
    if (MODE == 1) {
        u_h = ((float)s + u_h) / (float)samples;                            // jittered stratum s of n_t: two roundings
        const uint32_t h_t = wang_hash(t ^ wang_hash(g.seed ^ 0x9E3779B9u));    // the triangle's rotation
        const uint32_t k = s * 0x9E3779B9u + h_t;                          // wraps
        u_m = (float)(k >> 8) * 5.9604644775390625e-8f;                     // 24 bits x 2^-24: exact
    }
    float ta = random_float(rng);
    float tb = random_float(rng);
    if (ta + tb > 1.0f) { ta = 1.0f - ta; tb = 1.0f - tb; }
    const float4 v0 = g.gtris[(size_t)t * 3 + 0], e1 = g.gtris[(size_t)t * 3 + 1], e2 = g.gtris[(size_t)t * 3 + 2];
    const float px = (v0.x + ta * e1.x) + tb * e2.x;
    const float py = (v0.y + ta * e1.y) + tb * e2.y;
    const float pz = (v0.z + ta * e1.z) + tb * e2.z;
    const float sx = g.tx - g.fx, sy = g.ty - g.fy, sz = g.tz - g.fz;
    const float ox = g.fx + u_m * sx;
    const float oy = (g.fy + u_h * g.light_length) + u_m * sy;
    const float oz = g.fz + u_m * sz;
    const float dx = px - ox, dy = py - oy, dz = pz - oz;
    const float r = sqrtf((dx * dx + dy * dy) + dz * dz);
    double nx, ny, nz;
    const double nn = tri_normal(e1, e2, nx, ny, nz);
    const double Dx = (double)dx, Dy = (double)dy, Dz = (double)dz;
    const double R2 = Dx * Dx + Dy * Dy + Dz * Dz;
    const double R = sqrt(R2);
    double w = fabs(nx * Dx + ny * Dy + nz * Dz) / (nn * (R2 * R) * 12.566370614359172);
    float4 ray = make_float4(dx / r, dy / r, dz / r, oy);
    float tm = r * 0.9990234375f;
    if (!(r > 0.0f) || !(r <= 3.4028234663852886e38f)) {      // no direction: not traced (tmax 0 accepts no hit), weighs 0
        ray = make_float4(0.f, 1.f, 0.f, oy);
        tm = 0.0f;
        w = 0.0;
    }
    g.rays[i] = ray;
    g.oxz[i] = make_float2(ox, oz);
    g.tmax[i] = tm;
    g.w[i] = w;
}

void launch_refine_generate(const GatherGenParams& g, const int32_t* offs, int32_t lo, int32_t hi, int32_t rays, hipStream_t s)
{
    if (rays <= 0) return;
    const dim3 grid((unsigned)((rays + 255) / 256));
    if (g.mode == 1) hipLaunchKernelGGL((k_refine_generate<1>), grid, dim3(256), 0, s, g, offs, lo, hi, rays);
    else hipLaunchKernelGGL((k_refine_generate<0>), grid, dim3(256), 0, s, g, offs, lo, hi, rays);
}

// One thread per triangle of the chunk.  X1 and V1 are k_gather_reduce_var<MODE>'s expected and variance at S = n_t; the merge
// weighs the two estimates by their sample counts.
template <int MODE>
__global__ __launch_bounds__(256) void k_refine_reduce(const float4* __restrict__ gtris, const double* __restrict__ w,
                                                       const uint8_t* __restrict__ occluded, const int32_t* __restrict__ offs,
                                                       double* __restrict__ expected, double* __restrict__ variance,
                                                       int32_t first_tri, int32_t lo, int32_t hi, int32_t samples0,
                                                       int32_t photons_equiv)
{
    static_assert(MODE == 0 || MODE == 1, "gather sampling: independent or stratified");
    const int i = lo + (int)(blockIdx.x * 256 + threadIdx.x);
    if (i >= hi) return;
    const int32_t samples = offs[i + 1] - offs[i];
    if (samples == 0) return;                                  // every bit of both planes stays
    const size_t t = (size_t)first_tri + (size_t)i;
    double nx, ny, nz;
    const double nn = tri_normal(gtris[t * 3 + 1], gtris[t * 3 + 2], nx, ny, nz);
    double sum = 0.0;
    const size_t at = (size_t)(offs[i] - offs[lo]);
    for (int32_t s = 0; s < samples; ++s) sum = sum + (occluded[at + s] ? 0.0 : w[at + s]);
    const double c = (double)photons_equiv * (0.5 * nn);
    const double m = sum / (double)samples;
    const double X1 = nn == 0.0 ? 0.0 : c * m;
    double q = 0.0;
    if (MODE == 0) {
        for (int32_t s = 0; s < samples; ++s) {
            const double d = (occluded[at + s] ? 0.0 : w[at + s]) - m;
            q = q + d * d;
        }
    } else {
        double prev = occluded[at] ? 0.0 : w[at];
        for (int32_t s = 1; s < samples; ++s) {
            const double x = occluded[at + s] ? 0.0 : w[at + s];
            const double d = x - prev;
            q = q + d * d;
            prev = x;
        }
    }
    const double SS = (double)samples * (double)(samples - 1);
    const double v = MODE == 0 ? q / SS : q / (2.0 * SS);
    const double V1 = nn == 0.0 ? 0.0 : (c * c) * v;
    const double X0 = expected[t], V0 = variance[t];
    const double a = (double)samples0, b = (double)samples, tot = a + b;
    expected[t] = (a * X0 + b * X1) / tot;
    variance[t] = ((a * a) * V0 + (b * b) * V1) / (tot * tot);
}

void launch_refine_reduce(const float4* gtris, const double* w, const uint8_t* occluded, const int32_t* offs, double* expected,
                          double* variance, int32_t first_tri, int32_t lo, int32_t hi, int32_t samples0, int32_t photons_equiv,
                          int32_t mode, hipStream_t s)
{
    if (hi <= lo) return;
    const dim3 grid((unsigned)((hi - lo + 255) / 256));
    if (mode == 1) hipLaunchKernelGGL((k_refine_reduce<1>), grid, dim3(256), 0, s, gtris, w, occluded, offs, expected, variance,
                                      first_tri, lo, hi, samples0, photons_equiv);
    else hipLaunchKernelGGL((k_refine_reduce<0>), grid, dim3(256), 0, s, gtris, w, occluded, offs, expected, variance, first_tri, lo,
                            hi, samples0, photons_equiv);
}

}  // namespace uvrt

/*
 * uvrt.h -- C ABI of the MI355X (gfx950) UV-dose hot path.
 *
 * This is the drop-in boundary: the entry points below are what the reference's
 * `RayTracer` (raytracer.h:13-59, raytracer.cpp) needs in place of its OpenCL wrapper
 * (`Kernel`/`Buffer`, template/precomp.h:1239-1325).  Plain pointers and sizes only; every
 * call returns UVRT_OK (0) or a negative error code, and uvrt_last_error() returns the text.
 * A context is bound to one HIP device and one in-order HIP stream (the reference's single
 * in-order cl_command_queue, template/template.cpp:1446); calls are asynchronous unless they
 * read back to the host.  Not thread-safe per context (the reference is single-threaded).
 *
 * Record layouts handed over by the host are the reference's own:
 *   Tri      64 B  v0.xyz,pad,v1.xyz,pad,v2.xyz,pad,centroid.xyz,pad   (mesh.h:6-13, cl/tools.cl:31-37)
 *   BVHNode  32 B  min.xyz,leftFirst,max.xyz,triCount                  (bvh.h:11-21, cl/tools.cl:39-45)
 *   triIdx   u32[T]                                                    (bvh.h:45)
 *   Ray      32 B  dir.xyz,orig.xyz,dist,triID                         (cl/tools.cl:8-14)
 * Inside the context they are re-laid-out for the GPU.
 */
#ifndef UVRT_H
#define UVRT_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct uvrt_ctx uvrt_ctx;

enum {
    UVRT_OK = 0,
    UVRT_ERR_INVALID = -1,   /* bad argument / call order */
    UVRT_ERR_HIP = -2,       /* a HIP runtime call failed */
    UVRT_ERR_NO_DEVICE = -3, /* no usable gfx950 device */
    UVRT_ERR_BVH = -4,       /* malformed BVH (cycle, out-of-range child, leaf beyond triIdx) */
    UVRT_ERR_STACK = -5      /* traversal needed more than 32 stack entries (extend.cl:43) */
};

/* which per-triangle map computeDosage reads (raytracer.cpp:96-116) */
enum { UVRT_MAP_SUM = 0, UVRT_MAP_MAX = 1 };

const char* uvrt_last_error(void);
const char* uvrt_version(void);

/* Kernel::InitCL + the six `new Kernel(...)` of RayTracer::Init (myapp.cpp:21,
 * raytracer.cpp:17-22).  A new context starts with SEED = 0, like a freshly built
 * generate.cl program (generate.cl:6). */
int uvrt_create(int device_id, uvrt_ctx** out);
void uvrt_destroy(uvrt_ctx* ctx);

/* Use an externally owned hipStream_t (e.g. torch's current stream) instead of the context's
 * own.  NULL restores the context's own stream. */
int uvrt_set_stream(uvrt_ctx* ctx, void* hip_stream);

/* verticesBuffer / bvhNodesBuffer / triIdxBuffer upload (raytracer.cpp:24-30); callable again
 * at any time (CalibratePower swaps scenes, raytracer.cpp:166-187,212-224).  The arrays are
 * copied; the caller keeps ownership.  (Re)allocates and zeroes the per-triangle maps
 * (raytracer.cpp:32-35) when tri_count changes. */
int uvrt_set_scene(uvrt_ctx* ctx, const void* tris64, int32_t tri_count,
                   const void* nodes32, int32_t node_count, const uint32_t* tri_idx);

/* rayBuffer = new Buffer(32 * photonCount) (raytracer.cpp:136-139); size_t arithmetic, so the
 * reference's int overflow at 2^26 photons does not exist here. */
int uvrt_resize_rays(uvrt_ctx* ctx, int64_t photon_count);

/* cl/reset.cl:4-26 over the current scene's triangles (raytracer.cpp:141-142) */
int uvrt_reset(uvrt_ctx* ctx, int32_t reset_color);

/* cl/generate.cl:8-40 for global ids [first_gid, first_gid+n) of a launch of any size, under
 * the pinned SEED semantics of SURVEY.md 8c: work-item 0 reads SEED_{k-1}, every other
 * work-item reads SEED_k; the context's SEED advances to SEED_k on every call (SEED_k is a
 * function of light_pos and SEED_{k-1} only, so ranks that generate disjoint gid ranges of the
 * same launch stay in step).  n <= the capacity set by uvrt_resize_rays. */
int uvrt_generate(uvrt_ctx* ctx, const float light_pos[3], float light_length,
                  int64_t first_gid, int64_t n);

/* cl/extend.cl:85-99 over the n rays of the last uvrt_generate: closest hit through the BVH,
 * then one increment of tempPhotonMap[triID] per hit.  After uvrt_generate_sweep or uvrt_write_free_rays ("free rays"
 * below) it runs the free-origin kernel instead. */
int uvrt_extend(uvrt_ctx* ctx, int64_t n);

/* cl/accumulate.cl:4-14 over tri_count triangles.  (A full-range accumulate is enqueued with the next call: a uvrt_shade
 * right behind it -- the host loop's order, myapp.cpp:159-160 -- runs both in one kernel; same arithmetic, same order.) */
int uvrt_accumulate(uvrt_ctx* ctx, float time_step, int32_t tri_count);

/* cl/shade.cl:23-41 (computeDosage) over tri_count triangles */
int uvrt_compute_dosage(uvrt_ctx* ctx, int32_t which_map, int32_t photons_per_light,
                        float scaled_power, int32_t tri_count);

/* cl/shade.cl:43-71 (dosageToColor) into the context's 9-float/triangle colour buffer (the
 * reference writes a GL VBO, raytracer.cpp:37,119) */
int uvrt_dosage_to_color(uvrt_ctx* ctx, float min_value, int32_t threshold_view,
                         int32_t tri_count);

/* RayTracer::Shade's kernel pair in one launch (raytracer.cpp:96-118): computeDosage followed by
 * dosageToColor over tri_count triangles, same arithmetic, the dose buffer is written as well */
int uvrt_shade(uvrt_ctx* ctx, int32_t which_map, int32_t photons_per_light, float scaled_power,
               float min_value, int32_t threshold_view, int32_t tri_count);

/* clFinish(Kernel::GetQueue()) (myapp.cpp:165, raytracer.cpp:202); also reports a traversal
 * stack overflow raised by any extend since the last sync. */
int uvrt_sync(uvrt_ctx* ctx);

/* dosageBuffer->CopyFromDevice() (raytracer.cpp:204-207), any range; synchronises. */
int uvrt_read_dosage(uvrt_ctx* ctx, float* out, int32_t first, int32_t count);
int uvrt_read_color(uvrt_ctx* ctx, float* out9, int32_t first, int32_t count);

/* ---- program-scope SEED of generate.cl (generate.cl:6,39) ---- */
int uvrt_get_seed(uvrt_ctx* ctx, uint32_t* seed);
int uvrt_set_seed(uvrt_ctx* ctx, uint32_t seed);
/* SEED_k from SEED_{k-1} and the lamp position, without launching (host-side RNG walk of
 * work-item 0); used to give every rank of a sharded job its place in the global launch
 * order. */
uint32_t uvrt_seed_next(const float light_pos[3], float light_length, uint32_t seed_prev);

/* Advance the context's SEED as a uvrt_generate at this lamp would, without launching (a rank of a
 * sharded job skipping a launch that another rank traces). */
int uvrt_advance_seed(uvrt_ctx* ctx, const float light_pos[3], float light_length);

/* Which outcome of generate.cl's SEED race (generate.cl:6,13,39: every work-item reads the
 * program-scope SEED, work-item 0 overwrites it at its end) and of its float -> uint conversion of a
 * negative seed sum (undefined in OpenCL C) the context reproduces:
 *   0 (default) = the canonical semantics of SURVEY.md 8c: serial work-item order -- work-item 0 reads
 *     SEED_{k-1}, every other work-item reads SEED_k -- and the conversion through int64 (x86-64);
 *   1 = "gfx950-ocl": what the reference's generate.cl, compiled unmodified by ROCm's OpenCL compiler,
 *     does on this GPU (measured, tests/test_gpu_reference_kernels.py): SEED is fetched through the
 *     scalar cache, so EVERY work-item of launch k reads SEED_{k-1}; v_cvt_u32_f32 turns a negative sum
 *     into 0.  With uvrt_set_flavour(ctx, 1) the whole pipeline then reproduces the reference's own
 *     kernel chain running live on the MI355X: counts bit for bit, dose within 1e-4. */
int uvrt_set_seed_mode(uvrt_ctx* ctx, int32_t mode);
uint32_t uvrt_seed_next_mode(const float light_pos[3], float light_length, uint32_t seed_prev,
                             int32_t seed_mode);

/* ---- free rays: every ray with an origin of its own ----
 * uvrt_generate makes the rays of one lamp column and the default traversal kernel relies on it.  The two calls below make
 * rays whose origins differ; the uvrt_extend that follows traces them with the free-origin kernel (same visit order, box
 * test, triangle test and deposit: (dist, triID) and the counts are bit-identical to the CPU restatement in flavours 0 and
 * 1) into the same tempPhotonMap, so uvrt_accumulate, uvrt_shade, uvrt_read_counts and uvrt_device_ptr work unchanged.
 * Flavour 2 is refused (UVRT_ERR_INVALID) for such a launch; uvrt_set_wide_bvh and uvrt_set_sort_bits are ignored by it;
 * uvrt_set_record_hits + uvrt_read_rays return every ray's own origin.  uvrt_trace_batch_launches ("batched tracing"
 * below) traces sweeps and stops side by side.  The {orig.x, orig.z} array and the kernel's per-scene records are
 * allocated by the first such call.
 *
 * uvrt_generate_sweep: generate for a lamp that moves from `from` to `to` at constant speed while it radiates.  Work-item
 * gid runs generate.cl:13-35 with lightPos = from under the SEED semantics of uvrt_generate (mode 0: work-item 0 reads
 * SEED_{k-1}, every other one SEED_k), then draws u = RandomFloat(&seed) and starts at
 *     orig.c = from.c + u * (to.c - from.c)                                    for c = x, z
 *     orig.y = (from.y + r1 * light_length) + u * (to.y - from.y)
 * each fl(a + fl(u * fl(b - a))) in strict f32; the direction is generate's.  SEED_k is work-item 0's RNG state after the
 * draw of u: a function of `from` and SEED_{k-1} only (uvrt_seed_next_sweep: host only, no GPU needed).  With
 * uvrt_set_seed_mode(ctx, 1) the call fails with UVRT_ERR_INVALID: that mode models the race of generate.cl alone. */
int uvrt_generate_sweep(uvrt_ctx* ctx, const float from[3], const float to[3], float light_length,
                        int64_t first_gid, int64_t n);
uint32_t uvrt_seed_next_sweep(const float from[3], float light_length, uint32_t seed_prev);
/* Like uvrt_write_rays, but every 32-byte Ray record keeps its own orig.xyz: n host records become "the last generate".
 * SEED is untouched. */
int uvrt_write_free_rays(uvrt_ctx* ctx, const void* rays32, int64_t n);

/* ---- shadow rays and the direct gather ----
 * A photon count does not reach the dim triangles: half the test room receives no photon of 2^21.  The gather turns the
 * question round -- stand on each triangle and ask how much of the lamp it sees -- and needs an occlusion query for it: a ray
 * with a maximum distance that stops at its first hit.  The shadow-ray kernel is the free-origin traversal with dist preset
 * to tmax, ended by the first accepted hit: exactly what extend.cl answers for a ray whose `dist` is preset (flavours 0 and 1;
 * flavour 2 is refused).  Every call below runs on the context's stream behind all outstanding launches, leaves SEED and
 * tempPhotonMap untouched and drops "the last generate": uvrt_extend / uvrt_read_rays before the next generate return
 * UVRT_ERR_INVALID.  The arrays and the scene's free records are allocated on first use.
 *
 * uvrt_gather_direct, for triangle t (index into tris64) of [first_tri, first_tri + tri_count) and sample s < S, j = t*S + s:
 *     rng = WangHash(j ^ WangHash(seed));  u_h, u_m, a, b = RandomFloat(&rng) x 4       (cl/tools.cl:2-4)
 *     if (a + b > 1) { a = 1 - a; b = 1 - b; }      p = (v0 + a*e1) + b*e2,  e1 = v1 - v0, e2 = v2 - v0        (f32)
 *     o = uvrt_generate_sweep's origin with r1 := u_h and u := u_m  (from == to: a stop)
 *     d = p - o,  r = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z),  dir = d / r,  tmax = r * (1 - 2^-10)
 * (the factor keeps the target triangle from shadowing itself; a sample with r not finite or not > 0 is not traced and weighs
 * 0).  The weight, in f64: n = cross(e1, e2), nn = |n|, D = (double)d, R2 = D.D, R = sqrt(R2),
 *     w = |n.D| / (nn * (R2*R) * 12.566370614359172)
 * and expected[t] = (double)photons_equiv * (0.5*nn) * (sum_s (occluded ? 0 : w) / (double)S), 0 where nn == 0: the expected
 * tempPhotonMap entry of a launch of photons_equiv photons.  Every operator one rounding, the sum in sample order, no
 * atomics: a pure function of the arguments, whatever the capacity (triangles go in chunks of floor(capacity / S)) or the
 * split into ranges.  A triangle that no BVH leaf holds has no estimate (0), as it has no photon.
 * UVRT_ERR_INVALID with nothing changed: flavour 2, no scene, a range outside [0, T], a limit of the struct, a null argument. */
/* test / interop hook: n 32-byte Ray records, rec.dist = tmax; out[i] = 1 when some triangle is hit with
 * 0.0001f < t < tmax.  Uploads, traces, reads back; synchronises.  n <= capacity. */
int uvrt_occluded(uvrt_ctx* ctx, const void* rays32, int64_t n, uint8_t* out);
typedef struct {
    float from[3], to[3];    /* from == to: a stop */
    float light_length;
    int32_t samples;         /* S in [1, 4096]; S <= capacity; T*S < 2^31 */
    uint32_t seed;
    int32_t photons_equiv;   /* N > 0: Shade's divisor for maps fed by this plane */
    int32_t reserved[2];
} uvrt_gather_params;
/* The gather sampling mode: how u_h and u_m above are formed.  A property of the context like uvrt_set_flavour: it survives
 * uvrt_set_scene, needs no device work and is read by uvrt_gather_direct alone (uvrt_occluded, the photon path and the plan
 * calls never look at it).  UVRT_GATHER_INDEPENDENT (default) is the rule above, bit for bit.  UVRT_GATHER_STRATIFIED keeps
 * the four draws, their order, (a, b) and everything after the origin, and replaces the two lamp coordinates of sample s:
 *     rng = WangHash(j ^ WangHash(seed));  xi_h, xi_m, a, b = RandomFloat(&rng) x 4      (xi_m is drawn and discarded)
 *     u_h = fl( fl((float)s + xi_h) / (float)S )                   jittered stratum s of the rod: u_h in [s/S, (s+1)/S]
 *     h_t = WangHash(t ^ WangHash(seed ^ 0x9E3779B9u))
 *     k   = s * 0x9E3779B9u + h_t                                  (uint32, wraps)
 *     u_m = (float)(k >> 8) * 2^-24                                exact: the golden-ratio Weyl sequence, rotated per triangle
 * The rod's visibility behind an occluder's edge is close to monotone in height, so one sample per stratum takes most of the
 * binary-visibility scatter out of a triangle's estimate; every stratum is uniform and h_t is a hash, so the
 * estimate is unbiased in the sense the independent one is.  With S = 1 at a stop both modes give the same bits (u_h =
 * fl(fl(0 + xi_h) / 1) = xi_h and u_m multiplies a zero segment).  Another value: UVRT_ERR_INVALID, the mode unchanged. */
enum { UVRT_GATHER_INDEPENDENT = 0, UVRT_GATHER_STRATIFIED = 1 };
int uvrt_set_gather_sampling(uvrt_ctx* ctx, int32_t mode);
int uvrt_get_gather_sampling(uvrt_ctx* ctx, int32_t* mode);
/* The variance plane: with uvrt_set_gather_variance(ctx, 1) uvrt_gather_direct also writes variance[first_tri .. first_tri +
 * tri_count), f64[T], an estimate of the variance of expected[t] from the same shadow rays.  A property of the context like
 * the sampling mode: default 0, survives uvrt_set_scene, needs no device work; a value other than 0 / 1 is UVRT_ERR_INVALID
 * with the state unchanged.  With the state off uvrt_gather_direct is the call above bit for bit and never touches the plane.
 * With it on, samples < 2 is UVRT_ERR_INVALID with nothing changed, expected[t] carries the same bits as with it off, and with
 * x_s = occluded ? 0 : w_s, `sum` and nn as above, m = sum / (double)S, c = (double)photons_equiv * (0.5*nn),
 * SS = (double)S * (double)(S-1):
 *     UVRT_GATHER_INDEPENDENT:  q = sum_{s=0}^{S-1} (x_s - m)*(x_s - m),            v = q / SS          (sample variance of the mean)
 *     UVRT_GATHER_STRATIFIED:   q = sum_{s=1}^{S-1} (x_s - x_{s-1})*(x_s - x_{s-1}),  v = q / (2.0 * SS)  (successive differences)
 *     variance[t] = (nn == 0) ? 0 : (c*c) * v
 * every operator one f64 rounding, the sums in sample order, no atomics: a pure function of the arguments like the expected
 * plane.  The successive-difference form suits one sample per stratum: the sample variance would charge the estimate for the
 * rod's own trend in height, which stratification has taken out; a single visibility edge of weight w contributes
 * w^2 / (2 S (S-1)), at least the true <= w^2 / (4 S^2), so the form is conservative there.  The estimate is for S >= 16: at
 * S = 4 about half of all bounds expected - 2 sqrt(variance) are 0.
 * The plane is allocated (zeroed) on first use and zeroed by uvrt_set_scene; uvrt_accumulate_expected zeroes
 * variance[0 .. tri_count) along with the expected plane when the plane exists, so a stale variance is never paired with a
 * later estimate.  uvrt_read_variance / uvrt_write_variance are uvrt_read_expected / uvrt_write_expected for this plane (the
 * write serves a caller who brings an estimate of their own). */
int uvrt_set_gather_variance(uvrt_ctx* ctx, int32_t on);
int uvrt_get_gather_variance(uvrt_ctx* ctx, int32_t* on);
int uvrt_read_variance(uvrt_ctx* ctx, double* out, int32_t first, int32_t count);
int uvrt_write_variance(uvrt_ctx* ctx, const double* in, int32_t first, int32_t count);
/* writes expected[first_tri .. first_tri + tri_count) */
int uvrt_gather_direct(uvrt_ctx* ctx, const uvrt_gather_params* params, int32_t first_tri, int32_t tri_count);
/* cl/accumulate.cl:4-14 with expected[t] in place of (double)tempPhotonMap[t]: photonMap += expected * (double)timeStep,
 * maxPhotonMap = max(maxPhotonMap, expected), then expected = 0.  An accumulate that uvrt_accumulate has deferred is
 * completed first, so the maps see launch order; uvrt_shade / uvrt_compute_dosage then work unchanged with
 * photons_per_light = photons_equiv, and one map may mix photon launches and gather launches. */
int uvrt_accumulate_expected(uvrt_ctx* ctx, float time_step, int32_t tri_count);
/* the expected plane, any range; synchronises.  uvrt_set_scene zeroes the plane. */
int uvrt_read_expected(uvrt_ctx* ctx, double* out, int32_t first, int32_t count);
/* test / interop hook: copies host values into expected[first .. first + count); synchronises.  What the direct gather
 * writes is one irradiance estimate; a caller may capture an estimate of their own (uvrt_plan_capture_expected). */
int uvrt_write_expected(uvrt_ctx* ctx, const double* in, int32_t first, int32_t count);

/* ---- adaptive gather: extra shadow rays for the triangles whose estimate is the least certain ----
 * uvrt_gather_direct spends the same S samples on every triangle; its variance plane says where they were too few.
 * uvrt_gather_refine draws n_t further samples for triangle t, chosen from (expected[t], variance[t]), and merges them into
 * both planes.
 *
 * What it works on: the context remembers the last successful uvrt_gather_direct that ran with the variance plane on -- its
 * range, S0 = samples, seed, sampling mode, from, to, light_length and photons_equiv.  Host state only: no device work, no
 * existing result changes.  The refined range lies inside the remembered one; geometry, photons_equiv, S0 and the mode are the
 * remembered call's (not the context's current sampling mode).  The remembered gather is forgotten by a successful refine (one
 * refine per gather), uvrt_gather_direct with the variance off, uvrt_accumulate_expected, uvrt_write_expected /
 * uvrt_write_variance and uvrt_set_scene; uvrt_plan_capture_expected, uvrt_occluded and the read calls leave it.
 *
 * The count rule, for t in the range, X0 = expected[t], V0 = variance[t], nn as above; f64, one rounding per operator:
 *     if (nn == 0 || !(X0 > 0) || !(V0 > 0) || X0 < min_expected)  n_t = 0
 *     else  r = rel_error * X0;  want = ceil((double)S0 * (V0 / (r * r) - 1.0))
 *           !(want >= 1): n_t = 0 (NaN included);  want >= max_extra: n_t = max_extra;
 *           otherwise n_t = the smallest power of two >= max(want, 2)
 * (S0 samples gave V0, so S0 + n samples of the same scatter give about V0 S0 / (S0 + n): `want` is the n that brings
 * sqrt(variance) / expected to rel_error.)  A triangle whose first pass saw no scatter (V0 = 0: every sample occluded, or all
 * equal) is never refined.
 * The extra samples of a triangle with n_t > 0 are, bit for bit, the samples uvrt_gather_direct would draw for triangle t with
 * samples = n_t, seed = params->seed and the remembered mode and lamp: j = t * n_t + s, and the stratified mode has n_t strata.
 * With x_s = occluded ? 0 : w_s, X1 and V1 are expected[t] and variance[t] as that call would write them, and in place
 *     a = (double)S0, b = (double)n_t, tot = a + b
 *     expected[t] = (a * X0 + b * X1) / tot
 *     variance[t] = ((a * a) * V0 + (b * b) * V1) / (tot * tot)
 * A triangle with n_t = 0 keeps every bit of both planes.  The result is a pure function of the planes and the arguments,
 * whatever the capacity (rays go in chunks of whole triangles, at most `capacity` each) or the cut of the range into calls.
 * Device path: count, an exclusive prefix sum, ONE read-back of the offsets (the call synchronises there), then per chunk
 * generate -> the shadow-ray kernel -> reduce; nothing is launched after the scan when no triangle wants a sample.
 * Like uvrt_gather_direct the call drops "the last generate" and leaves SEED and tempPhotonMap untouched.
 * UVRT_ERR_INVALID with nothing changed: no remembered gather, a range outside it, seed equal to the gather's, flavour 2, a
 * limit of the struct, a null context or params. */
typedef struct {
    double  rel_error;     /* tau: target sqrt(variance)/expected; finite, > 0 */
    double  min_expected;  /* triangles with expected < this are left alone; finite, >= 0 (0: none) */
    int32_t max_extra;     /* power of two in [2, 4096]; <= capacity; T * max_extra < 2^31 */
    uint32_t seed;         /* seed of the extra samples; must differ from the refined gather's seed */
    int32_t reserved[2];   /* 0 */
} uvrt_refine_params;
typedef struct { int64_t extra_rays; int32_t refined; int32_t reserved; } uvrt_refine_report;   /* sum of n_t; triangles with n_t > 0 */
int uvrt_gather_refine(uvrt_ctx* ctx, const uvrt_refine_params* params, int32_t first_tri, int32_t tri_count,
                       uvrt_refine_report* report /* may be NULL */);
/* test hook: n_t of the last uvrt_gather_refine, int32[T]; 0 outside its range (and before the first refine of a scene);
 * synchronises */
int uvrt_read_gather_extra(uvrt_ctx* ctx, int32_t* out, int32_t first, int32_t count);
/* test hook: the count rule and the prefix sum of uvrt_gather_refine alone, on the planes as they are.  uvrt_write_expected and
 * uvrt_write_variance forget the remembered gather, so a refine only ever counts on planes a gather left; this call runs the
 * same two device steps (the count, the three-pass scan) on whatever expected[] and variance[] hold, with S0 = samples0 in
 * [2, 4096] from the caller, over triangles [first_tri, first_tri + tri_count) of [0, T].  offsets_out[0 .. tri_count] receives
 * the exclusive prefix sum of n_t over the range (offsets_out[tri_count] is the total); n_t itself is what
 * uvrt_read_gather_extra then reads, 0 outside the range.  Synchronises.
 * It traces nothing and leaves both planes, the remembered gather, "the last generate", SEED and the maps as they are; planes
 * and per-triangle records that no call has made yet are made (the planes zeroed) as their read calls would.  params is checked
 * as uvrt_gather_refine checks it, but for the seed (no ray is drawn) and max_extra <= capacity (no ray is stored); there need
 * be no remembered gather.  UVRT_ERR_INVALID with nothing changed, the n_t plane included: those limits, samples0, a range
 * outside [0, T], flavour 2, no scene, a null argument. */
int uvrt_refine_counts(uvrt_ctx* ctx, int32_t samples0, const uvrt_refine_params* params, int32_t first_tri, int32_t tri_count,
                       int32_t* offsets_out /* tri_count + 1 */);

/* ---- batched direct gather: one shadow-ray pass for several launches ----
 * A gather launch on a room of 45 k triangles is a launch tail, not a traversal: at S = 16 it holds little more than one ray
 * per lane of the persistent query grid.  uvrt_gather_direct_batch traces `count` launches over one triangle range in one
 * pass and keeps their planes; uvrt_gather_batch_select then puts launch k's where uvrt_gather_direct would
 * have left them.  Every bit equals what the launch-by-launch calls give.
 *
 * uvrt_gather_direct_batch: count in [1, UVRT_GATHER_BATCH_MAX]; every launch is checked as uvrt_gather_direct checks it
 * (flavour 0 / 1, a scene, the range, S in [1, 4096], S <= capacity, T*S < 2^31, photons_equiv > 0, S >= 2 with the variance
 * state on), and all launches share one `samples`; from, to (stops and sweeps mix), light_length, seed and photons_equiv may
 * differ.  A refusal is UVRT_ERR_INVALID with nothing changed: an earlier batch is kept.  A call that passes drops the earlier
 * batch, records the context's sampling mode, variance state and flavour as they are now and makes E_b, f64[count][T] (and
 * V_b, the same shape, when the variance state is on): E_b[k][t] is the plane uvrt_gather_direct(&launches[k], first_tri,
 * tri_count) would leave in `expected`, V_b[k][t] in `variance`; entries outside the range are 0; tri_count = 0 is a valid empty
 * batch.  The unit of work is the pair q = k * tri_count + lt, launch-major; pairs go in chunks of floor(capacity / S) through
 * lane 0's ray buffers (a chunk may straddle a launch boundary), per chunk generate -> the shadow-ray kernel -> reduce, with the
 * sample rule and the sample-order sums above and no atomics: a pure function of the arguments and the recorded state,
 * whatever the capacity.  It runs on the context's stream behind all outstanding launches and, like every shadow-ray call,
 * drops "the last generate"; it leaves SEED, tempPhotonMap, expected, variance, source, the links and the remembered gather of
 * uvrt_gather_refine untouched.
 *
 * uvrt_gather_batch_select(k): expected[range] = E_b[k][range] -- and variance[range] = V_b[k][range] when the batch has a
 * variance plane, else that plane is not touched --, device to device on the stream; entries outside the range keep their bits.
 * The remembered gather becomes launch k's under the recorded mode when the batch has a variance plane, and is forgotten
 * otherwise: the context is as uvrt_gather_direct(&launches[k], ..) would have left it under the recorded state, so refine, both
 * bounces, uvrt_plan_capture_expected and uvrt_accumulate_expected follow unchanged.  Any k, in any order, repeatedly.
 * UVRT_ERR_INVALID with nothing changed: no batch, k outside [0, count).
 * A batch survives every call but uvrt_set_scene, the next successful uvrt_gather_direct_batch and uvrt_destroy (the refine and
 * the bounces trace through lane 0's ray buffers, not the batch's planes). */
enum { UVRT_GATHER_BATCH_MAX = 64 };
/* E_b[k][t], k < count: the plane uvrt_gather_direct(&launches[k], first_tri, tri_count) would leave in `expected`
 * (and V_b[k][t] its variance plane when uvrt_set_gather_variance is on), all traced in one pass */
int uvrt_gather_direct_batch(uvrt_ctx* ctx, const uvrt_gather_params* launches, int32_t count,
                             int32_t first_tri, int32_t tri_count);
int uvrt_gather_batch_select(uvrt_ctx* ctx, int32_t k);
int uvrt_gather_batch_info(uvrt_ctx* ctx, int32_t out4[4]);   /* {count (0: no batch), samples, first_tri, tri_count} */
/* test hook: which = 0 expected, 1 variance (UVRT_ERR_INVALID for a batch without one); any range of [0, T); synchronises */
int uvrt_read_gather_batch(uvrt_ctx* ctx, int32_t k, int32_t which, double* out, int32_t first, int32_t count);

/* ---- one diffuse bounce: a closest-hit query and a final gather over a per-triangle source plane ----
 * The direct gather sees the lamp alone; light that arrives by reflection it cannot see.  uvrt_gather_indirect adds one
 * bounce as a final gather: from points on triangle t it shoots cosine-distributed rays, finds the closest hit and looks up
 * what the hit triangle already receives in a third plane, `source`, f64[T].  The query is the free-origin
 * traversal with dist preset to tmax that runs to the end of its stack and deposits nothing: what extend.cl leaves in
 * ray->dist / ray->triID for that preset (flavours 0 and 1; flavour 2 is refused).  Like the shadow-ray calls, every tracing
 * call below runs on the context's stream behind all outstanding launches, leaves SEED and tempPhotonMap untouched and drops
 * "the last generate".
 *
 * The source plane holds, for ALL T triangles, the expected tempPhotonMap entry that acts as the emitter -- normally a
 * snapshot of a finished direct gather (uvrt_indirect_source_from_expected).  It is allocated (zeroed) on first use, zeroed
 * by uvrt_set_scene, and is uvrt_device_ptr(ctx, 8, ...).  uvrt_read_indirect_source / uvrt_write_indirect_source are
 * uvrt_read_expected / uvrt_write_expected for this plane: the write serves a caller who wants further bounces or a
 * reflectance per triangle (scale the plane).
 *
 * uvrt_gather_indirect reads source[0..T) and writes only expected[first_tri .. first_tri + tri_count).  For triangle t of the
 * range and sample s < S2, j = t*S2 + s (uint32); f32 and f64 as marked, every operator one rounding:
 *     rng = WangHash(j ^ WangHash(seed));  a, b = RandomFloat(&rng) x 2;  if (a + b > 1) { a = 1 - a; b = 1 - b; }      (f32)
 *     p.c = (v0.c + a*e1.c) + b*e2.c                                                the gather's point
 *     up to 8 rounds:  xf, yf = RandomFloat x 2;  x = (double)(xf*2.0f - 1.0f), y likewise;  accept when x*x + y*y <= 1.0
 *                      after 8 rejected rounds: x = y = 0                           (generate.cl:25-28's disc, bounded)
 *     n = cross(e1, e2), nn = |n|  (f64);  E = (double)e1;  l1 = sqrt((E.x*E.x + E.y*E.y) + E.z*E.z);  T = E / l1
 *     B.x = (n.y*T.z - n.z*T.y) / nn,  B.y = (n.z*T.x - n.x*T.z) / nn,  B.z = (n.x*T.y - n.y*T.x) / nn
 *     z = sqrt(1.0 - (x*x + y*y));  zz = ((s & 1) ? -z : z) / nn        odd samples leave the other face: the model is two-sided
 *     D.c = ((x*T.c) + (y*B.c)) + (zz*n.c);  dir.c = (float)D.c
 *     ray: orig = p, dir, tmax = 1e30f.  Not traced (dir = (0,1,0), tmax = 0): nn == 0, a dir component not finite, or all zero
 *     h_s = the closest hit's triangle;  y_s = (hit && h_s != t && nn_h > 0) ? source[h_s] / (0.5*nn_h) : 0.0
 *     ind[t] = (nn == 0) ? 0 : ((double)rho * (0.5*nn)) * ((2.0 * sum_s y_s) / (double)S2)      sum in sample order, no atomics
 *     expected[t] = add ? expected[t] + ind[t] : ind[t]
 * Directions (x, y, sqrt(1 - x^2 - y^2)) over a uniform disc are cosine-distributed, so the irradiance a Lambertian surround of
 * radiosity rho*e' sends to p is rho x the mean of e' over a hemisphere's samples; S2/2 samples go to each face and the faces
 * add, hence 2/S2.  The units are those of `expected`.  A pure function of the source plane, the range's own expected values
 * (when add) and the arguments, whatever the capacity (triangles go in chunks of floor(capacity / S2)) or the cut of the range
 * into calls.  Device path per chunk: generate -> the closest-hit kernel -> reduce.
 * The call leaves `source` and the variance plane untouched and forgets the remembered gather of uvrt_gather_refine, as
 * uvrt_write_expected does; uvrt_indirect_source_from_expected and the read calls leave it.
 * Limits: one bounce; rho uniform; a single-sheet object lit on one face re-emits from both (at most a factor rho); the
 * variance plane is the direct part's.
 * UVRT_ERR_INVALID with nothing changed: a null argument, no scene, flavour 2, a range outside [0, T], odd or out-of-range
 * samples, reflectance outside [0, 1] or not finite, add other than 0 / 1, non-zero reserved, the limits of the struct. */
/* test / interop hook, the closest-hit twin of uvrt_occluded: n 32-byte Ray records with origins of their own, rec.dist = tmax
 * (1e30f: none).  dist_out[i] / tri_out[i] = what extend.cl leaves in ray->dist / ray->triID for that preset, tri_out = -1 and
 * dist_out = tmax (same bits) when nothing is accepted.  Flavours 0 and 1; n <= capacity; uploads, traces, reads back,
 * synchronises; leaves SEED and tempPhotonMap untouched and drops "the last generate", like uvrt_occluded. */
int uvrt_closest_hits(uvrt_ctx* ctx, const void* rays32, int64_t n, float* dist_out, int32_t* tri_out);

typedef struct {
    float    reflectance;   /* rho: finite, in [0, 1] */
    int32_t  samples;       /* S2: EVEN, in [2, 4096]; <= capacity; T * S2 < 2^31 */
    uint32_t seed;
    int32_t  add;           /* 0: expected[t] = ind[t];  1: expected[t] = expected[t] + ind[t] */
    int32_t  reserved[2];   /* 0 */
} uvrt_indirect_params;
/* source[0..T) = expected[0..T), on the stream; both planes made if absent */
int uvrt_indirect_source_from_expected(uvrt_ctx* ctx);
int uvrt_read_indirect_source(uvrt_ctx* ctx, double* out, int32_t first, int32_t count);
int uvrt_write_indirect_source(uvrt_ctx* ctx, const double* in, int32_t first, int32_t count);
int uvrt_gather_indirect(uvrt_ctx* ctx, const uvrt_indirect_params* params, int32_t first_tri, int32_t tri_count);
/* test hook: the rays uvrt_gather_indirect would trace for the range (its generate kernel alone, chunked the same way),
 * as 32-byte Ray records with dist = tmax; synchronises; changes no plane */
int uvrt_gather_indirect_rays(uvrt_ctx* ctx, const uvrt_indirect_params* params, int32_t first_tri, int32_t tri_count,
                              void* rays32_out);

/* ---- recorded hit links: the bounce's rays traced once per scene, and gathers of several bounces over them ----
 * The rays of uvrt_gather_indirect are a function of the scene, S2 and the seed alone; only the `source` values looked up at
 * their hits change from launch to launch.  uvrt_indirect_links_build traces them once, for ALL T triangles, and records for
 * every (triangle t, sample s) the hit link
 *     link[t][s] = (hit && h_s != t && nn_h > 0) ? h_s : -1
 * with h_s as above: the condition under which y_s can be non-zero is baked into the link.  It runs on the context's stream
 * behind all outstanding launches, in chunks of floor(capacity / S2) triangles, each chunk generate -> the closest-hit kernel
 * (as uvrt_gather_indirect, with the same sample numbers and WangHash(seed)) -> a store kernel.  Like uvrt_gather_indirect it
 * drops "the last generate" and leaves SEED, tempPhotonMap and every plane untouched; it also leaves the remembered gather of
 * uvrt_gather_refine.  A second build replaces the links, uvrt_set_scene drops them, uvrt_set_flavour leaves them:
 * uvrt_indirect_links_info reports {samples (0: no links), seed, the flavour they were traced in, the kind (0: these links; 1: sided ones,
 * "face-resolved gather and bounces" below)}.
 * UVRT_ERR_INVALID with nothing changed and earlier links kept: a null argument, no scene, flavour 2, non-zero reserved, and
 * what uvrt_gather_indirect refuses for `samples`.  A failed allocation: UVRT_ERR_HIP, earlier links kept.
 * uvrt_read_indirect_links (test hook; synchronises): out[(t - first_tri) * S2 + s] = link[t][s], whatever the device layout
 * (which is sample-major).
 *
 * uvrt_gather_indirect_linked reads source[0..T) and the links and writes only expected[first_tri .. first_tri + tri_count).
 * K = bounces in [1, 16]; everything f64, every operator one rounding, nn_t = |cross(e1, e2)| as above:
 *     e_0[h] = nn_h > 0 ? source[h] / (0.5*nn_h) : 0.0                                                       all h
 *     for b = 1..K:
 *       g_b[t] = nn_t == 0 ? 0.0 : ((double)rho * (0.5*nn_t)) * ((2.0 * sum_s (link[t][s] >= 0 ? e_{b-1}[link[t][s]] : 0.0)) / (double)S2)
 *       e_b[t] = nn_t > 0 ? g_b[t] / (0.5*nn_t) : 0.0
 *     total[t]    = (..((g_1[t] + g_2[t]) + g_3[t]) .. + g_K[t])             ascending b; K = 1: g_1[t]
 *     expected[t] = add ? expected[t] + total[t] : total[t]
 * The sum over s runs in sample order from +0.0, without atomics.  These are uvrt_gather_indirect's expressions: with K = 1
 * and links built with (S2, seed) in flavour f the call gives `expected` bit for bit what uvrt_gather_indirect(rho, S2, seed,
 * add) gives in flavour f.  Bounces before the last are evaluated for all T triangles (they are the next bounce's source), so
 * a triangle's result depends neither on the range nor on its cut into calls.  The call traces nothing: it works in any
 * flavour, runs on the context's stream behind all outstanding launches (one kernel launch per bounce), leaves "the last
 * generate", SEED, tempPhotonMap, `source`, the variance plane and the links untouched and forgets the remembered gather of
 * uvrt_gather_refine, as uvrt_write_expected does.
 * What is traded: every launch sees the same directions, so the bounce's sampling error is common to all
 * launches of a route and does not average out over them; S2 is paid once per scene and can be chosen much larger.
 * UVRT_ERR_INVALID with nothing changed: a null argument, no scene, no links, bounces outside [1, 16], reflectance outside
 * [0, 1] or not finite, add other than 0 / 1, non-zero reserved, a range outside [0, T]. */
typedef struct {
    int32_t  samples;       /* S2: as for uvrt_indirect_params */
    uint32_t seed;
    int32_t  reserved[2];   /* 0 */
} uvrt_links_params;
int uvrt_indirect_links_build(uvrt_ctx* ctx, const uvrt_links_params* params);
int uvrt_indirect_links_info(uvrt_ctx* ctx, int32_t out4[4]);
int uvrt_read_indirect_links(uvrt_ctx* ctx, int32_t* out, int32_t first_tri, int32_t tri_count);
typedef struct {
    float    reflectance;   /* rho: finite, in [0, 1] */
    int32_t  bounces;       /* K: in [1, 16] */
    int32_t  add;           /* 0: expected[t] = total[t];  1: expected[t] = expected[t] + total[t] */
    int32_t  reserved[3];   /* 0 */
} uvrt_linked_params;
int uvrt_gather_indirect_linked(uvrt_ctx* ctx, const uvrt_linked_params* params, int32_t first_tri, int32_t tri_count);

/* ---- face-resolved gather and bounces: every triangle an opaque sheet whose two faces keep their own irradiance ----
 * The bounces above are two-sided: a triangle gathers over both hemispheres and what arrives on either face is re-emitted
 * from both, so the bounce operator can have a gain above 1 and the series g_1 + g_2 + .. need not converge.
 * The calls below resolve the faces instead: light that arrives on a face is re-emitted from that face only, and a
 * ray that leaves face f of triangle t and arrives on face a of triangle h looks up what face a of h receives.  No notion of
 * "inside" is needed: the arrival face is the sign of n_h . dir.  Everything here is additive: `expected`, the photon path and
 * every call above keep their bits.
 *
 * Face convention: face 0 of triangle t is the side n = cross(e1, e2) points to.  A ray travelling along v arrives on face 0
 * iff n.v < 0, on face 1 otherwise.  Even samples of the bounce leave face 0 and odd samples face 1 (`zz` above).
 *
 * The direct gather's face planes.  uvrt_set_gather_faces is a property of the context like uvrt_set_gather_variance: default
 * 0, survives uvrt_set_scene, needs no device work; a value other than 0 / 1 is UVRT_ERR_INVALID with the state unchanged.  With
 * the state off uvrt_gather_direct launches what it launches without it and makes no buffer.  With it on the call also writes
 * faces[f][t], f64[2][T], for t in the range; in the notation of uvrt_gather_direct, for sample s
 *     c_s = (n.x*D.x + n.y*D.y) + n.z*D.z          the f64 value the weight takes fabs of
 *     f_s = c_s < 0 ? 0 : 1,     x_s = occluded ? 0 : w_s
 *     faces[f][t] = nn == 0 ? 0 : ((double)photons_equiv * (0.5*nn)) * ((sum_{s : f_s = f} x_s) / (double)S)
 * the sum in sample order from +0.0, no atomics (every term is >= +0, so skipping the other face's samples and adding +0.0
 * for them give the same bits).  expected[t] and variance[t] carry the bits they carry with the state off; when every visible
 * sample of a triangle lies on one face, that face's entry equals expected[t] bit for bit and the other is +0.0.  The planes
 * are allocated (zeroed) on first use and zeroed by uvrt_set_scene; uvrt_accumulate_expected zeroes faces[.][0 .. tri_count)
 * when they exist, as it does for the variance.  uvrt_gather_refine, uvrt_gather_indirect*, uvrt_write_expected and
 * uvrt_gather_batch_select leave them alone: after a refine the planes describe the first pass.  uvrt_gather_direct_batch with
 * the state on is UVRT_ERR_INVALID with nothing changed and an earlier batch kept (a batch keeps no face planes).
 * uvrt_read_gather_faces / uvrt_write_gather_faces: a range of plane `face` (0 / 1, else UVRT_ERR_INVALID) as
 * uvrt_read_variance / uvrt_write_variance; they synchronise; the write serves tests and a caller with an emitter of their own
 * and, touching neither plane a refine works on, leaves the remembered gather.  The planes are not a uvrt_device_ptr index. */
int uvrt_set_gather_faces(uvrt_ctx* ctx, int32_t on);
int uvrt_get_gather_faces(uvrt_ctx* ctx, int32_t* on);
int uvrt_read_gather_faces(uvrt_ctx* ctx, int32_t face, double* out, int32_t first, int32_t count);
int uvrt_write_gather_faces(uvrt_ctx* ctx, int32_t face, const double* in, int32_t first, int32_t count);
/* Sided links.  uvrt_indirect_links_build_sided is uvrt_indirect_links_build in everything -- the same rays, chunks, refusals
 * and lifecycle, built into a buffer of its own and swapped in at the end -- but for the stored value:
 *     link[t][s] = keep ? (h_s << 1) | a_s : -1        keep: the filter of the plain link (hit && h_s != t && nn_h > 0)
 *     a_s = c < 0 ? 0 : 1,   c = (n_h.x*(double)dir.x + n_h.y*(double)dir.y) + n_h.z*(double)dir.z
 * with n_h = cross(e1, e2) of h_s in f64 and dir the f32 direction of the sample (uvrt_gather_indirect_rays).  For the same
 * (S2, seed, flavour) link >> 1 is the plain link wherever it is >= 0, and -1 sits in the same places.  A context holds one
 * link set: a plain build replaces sided links and the other way round; uvrt_indirect_links_info reports the kind in out4[3]
 * (0 plain, 1 sided) and uvrt_read_indirect_links returns the stored values as they are.  uvrt_gather_indirect_linked on sided
 * links and uvrt_gather_indirect_linked_sided on plain ones are UVRT_ERR_INVALID with nothing changed.
 *
 * uvrt_gather_indirect_linked_sided: the struct, the checks and K in [1, 16] of uvrt_gather_indirect_linked.  It reads
 * faces[2][T] as the emitter (no snapshot; made zeroed when absent; never written) and the sided links, and writes only
 * expected[first_tri .. first_tri + tri_count).  Everything f64, every operator one rounding, L = link[t][s]:
 *     e_0[f][h] = nn_h > 0 ? faces[f][h] / (0.5*nn_h) : 0.0                                      f = 0, 1; all h
 *     for b = 1..K, f = 0, 1:
 *       g_b[f][t] = nn_t == 0 ? 0.0
 *                 : ((double)rho * (0.5*nn_t)) * ((2.0 * sum_{s = f, f+2, .. < S2} (L >= 0 ? e_{b-1}[L & 1][L >> 1] : 0.0)) / (double)S2)
 *       e_b[f][t] = nn_t > 0 ? g_b[f][t] / (0.5*nn_t) : 0.0
 *     G_b[t]      = g_b[0][t] + g_b[1][t]
 *     total[t]    = (..((G_1[t] + G_2[t]) + G_3[t]) .. + G_K[t])
 *     expected[t] = add ? expected[t] + total[t] : total[t]
 * Each face has S2/2 cosine samples over its own hemisphere, hence 2/S2 (S2 is even).  The sums run in ascending s from +0.0,
 * without atomics.  Bounces before the last are evaluated for all T triangles, so the result depends neither on the range nor
 * on its cut into calls.  max e_b <= rho * max e_{b-1} up to rounding, so the series converges for every rho <= 1.  The call
 * traces nothing, works in any flavour (one plain kernel launch per bounce) and leaves and forgets exactly what
 * uvrt_gather_indirect_linked leaves and forgets. */
int uvrt_indirect_links_build_sided(uvrt_ctx* ctx, const uvrt_links_params* params);
int uvrt_gather_indirect_linked_sided(uvrt_ctx* ctx, const uvrt_linked_params* params, int32_t first_tri, int32_t tri_count);

/* ---- per-face reflectance: the face-resolved bounces with a reflectance map instead of one rho ----
 * The reflectance planes.  rho[f][t], f32[2][T], plane-major like `faces`: the diffuse reflectance of face f of triangle t, in
 * the face convention above (face 0 is the side cross(e1, e2) points to).  A scene has no planes until a call below makes them;
 * uvrt_set_scene drops them and every other call above leaves them bit for bit.  They are not a uvrt_device_ptr index.
 *   uvrt_fill_reflectance   makes the planes if absent and sets all 2*T entries to rho (on the stream, behind outstanding work).
 *   uvrt_write_reflectance  makes the planes if absent -- zeroed, so an unlisted face absorbs everything and never overstates
 *                           a dose -- then writes [first, first + count) of plane `face`; synchronises, like
 *                           uvrt_write_gather_faces.
 *   uvrt_read_reflectance   the same range back; UVRT_ERR_INVALID when there are no planes ("no map" is not "rho = 0").
 *   uvrt_reflectance_info   *have = 1 when the scene has planes, else 0.
 *   uvrt_drop_reflectance   frees them (nothing to do when there are none).
 * Every value must be finite and in [0, 1]; the host checks the whole input before anything is uploaded.  A bad value, a face
 * other than 0 / 1, a range outside [0, T), a null argument or no scene: UVRT_ERR_INVALID with nothing changed, and planes that
 * did not exist are not made.
 *
 * uvrt_gather_indirect_linked_mapped reads faces[2][T] (made zeroed when absent, never written), the SIDED links and rho, and
 * writes only expected[first_tri .. first_tri + tri_count).  Everything f64, every operator one rounding, L = link[t][s],
 * nn_t = |cross(e1, e2)|:
 *     e_0[f][h] = nn_h > 0 ? faces[f][h] / (0.5*nn_h) : 0.0                                      f = 0, 1; all h
 *     r_b[f][h] = (double)rho[f][h] * e_b[f][h]                                                   what face f of h sends back
 *     for b = 1..K, f = 0, 1:
 *       g_b[f][t] = nn_t == 0 ? 0.0
 *                 : (0.5*nn_t) * ((2.0 * sum_{s = f, f+2, .. < S2} (L >= 0 ? r_{b-1}[L & 1][L >> 1] : 0.0)) / (double)S2)
 *       e_b[f][t] = nn_t > 0 ? g_b[f][t] / (0.5*nn_t) : 0.0
 *     G_b[t]      = g_b[0][t] + g_b[1][t]
 *     total[t]    = (..((G_1[t] + G_2[t]) + G_3[t]) .. + G_K[t])
 *     expected[t] = add ? expected[t] + total[t] : total[t]
 * The reflectance belongs to the face that EMITS -- the face the link arrives on -- not to the receiver: with one rho the two
 * placements are the same number, with a map only this one is physics.  The sums run in ascending s from +0.0, without atomics;
 * bounces before the last are evaluated for all T triangles, so the result depends neither on the range nor on its cut into
 * calls; max e_b <= max rho * max e_{b-1} up to rounding.  With rho == 1.0f everywhere `total` is that of
 * uvrt_gather_indirect_linked_sided(reflectance = 1) bit for bit (1.0*x is exact); with any other constant c the two differ by
 * rounding alone: |mapped / sided - 1| <= K * (S2 + 16) * 2^-53 wherever the sided value is > 0, zeros in the same places.
 * The call traces nothing, works in any flavour (one plain kernel launch per bounce), leaves and forgets exactly what
 * uvrt_gather_indirect_linked_sided leaves and forgets, and leaves rho.
 * UVRT_ERR_INVALID with nothing changed: a null argument, no scene, no links, plain links, no reflectance planes, bounces
 * outside [1, 16], add other than 0 / 1, non-zero reserved, a range outside [0, T]. */
int uvrt_fill_reflectance(uvrt_ctx* ctx, float rho);
int uvrt_write_reflectance(uvrt_ctx* ctx, int32_t face, const float* in, int32_t first, int32_t count);
int uvrt_read_reflectance(uvrt_ctx* ctx, int32_t face, float* out, int32_t first, int32_t count);
int uvrt_reflectance_info(uvrt_ctx* ctx, int32_t* have);
int uvrt_drop_reflectance(uvrt_ctx* ctx);
typedef struct {
    int32_t  bounces;       /* K: in [1, 16] */
    int32_t  add;           /* 0: expected[t] = total[t];  1: expected[t] = expected[t] + total[t] */
    int32_t  reserved[2];   /* 0 */
} uvrt_mapped_params;
int uvrt_gather_indirect_linked_mapped(uvrt_ctx* ctx, const uvrt_mapped_params* params, int32_t first_tri, int32_t tri_count);

/* ---- specular panels: the mirror-image gather of the lamp ----
 * Everything above is diffuse.  A polished panel does not spread the lamp's light over the hemisphere: it shows every surface
 * in front of it a second lamp behind the wall.  For a planar panel the path lamp -> panel -> surface has a closed form, the
 * image method: the receiver sees the lamp point mirrored in the panel's plane, at the unfolded distance, provided the mirror
 * point lies on the panel, the lamp sees the mirror point and the mirror point sees the receiver.  Everything here is
 * additive: with no panels set every call above keeps its bits.
 *
 * Panels.  Panel k is an ideal plane (point q, normal m) with a specular reflectance rho_k in [0, 1]; it reflects on the side m
 * points to.  panel_of_tri[t], uint8[T], is 0 (no mirror) or k + 1: the plane carries the optics, the member triangles say
 * where the plane is a mirror (and occlude like every triangle).  uvrt_set_mirrors validates everything on the host before
 * anything is uploaded -- count outside [1, UVRT_MIRROR_MAX], a non-finite value, |m| = 0, rho outside [0, 1], reserved != 0,
 * an entry of panel_of_tri above count, no scene, a null argument: UVRT_ERR_INVALID with nothing changed -- forms
 * mh = m / |m| in f64 (|m| = sqrt((m.x*m.x + m.y*m.y) + m.z*m.z) of the (double) components) and keeps it with (double)q.  A
 * second call replaces the first.  The panels belong to the scene: uvrt_set_scene and uvrt_drop_mirrors drop them, every other
 * call leaves them bit for bit; they are not a uvrt_device_ptr index.  uvrt_mirror_info: out4 = {count (0: none), member
 * triangles, 0, 0}.  uvrt_read_mirrors: the records as they were set and panel_of_tri as the kernels read it; UVRT_ERR_INVALID
 * when there are none.
 *
 * uvrt_gather_mirror, for panel k = 0 .. count-1 in order, triangle t of the range and sample s < S = params->samples, in the
 * notation of uvrt_gather_direct and under the context's sampling mode (the draws, p and o are uvrt_gather_direct's, sample for
 * sample; flavours 0 and 1):
 *     d_o = (((double)o.x - q.x)*mh.x + ((double)o.y - q.y)*mh.y) + ((double)o.z - q.z)*mh.z,   d_p likewise from p      (f64)
 *     unless d_o > 0 and d_p > 0 the sample weighs 0 and is not traced (ray (0,1,0), tmax 0)
 *     o' = (float)((double)o - (2.0*d_o)*mh)                                    per component: the image of the lamp point
 *     D' = p - o' (f32), r' = sqrtf((D'.x*D'.x + D'.y*D'.y) + D'.z*D'.z);  r' not finite or not > 0: weighs 0, not traced
 *     c' = n.D',  w' = (double)rho_k * ( |c'| / (nn * (R2'*R') * 12.566370614359172) ),  face f_s = c' < 0 ? 0 : 1
 * (c' and the bracket are uvrt_gather_direct's own expressions with o' in place of o: one copy serves both gathers).
 *   Leg A, lamp to mirror point:  tau = d_o / (d_o + d_p),  P = (float)((double)o' + tau*(double)D'),  A = P - o (f32),
 *     r_A = sqrtf((A.x*A.x + A.y*A.y) + A.z*A.z); r_A not finite or not > 0: weighs 0, not traced.  Ray: origin o, direction
 *     A / r_A, tmax 1e30f; a closest-hit query (uvrt_closest_hits) answers (dist, h).  The sample is LOST unless h < T and
 *     panel_of_tri[h] == k + 1.
 *   Leg B, mirror point to receiver:  P_h = o + dist*(A / r_A),  B = p - P_h,  r_B = sqrtf((B.x*B.x + B.y*B.y) + B.z*B.z), all
 *     f32; r_B not finite or not > 0: lost.  Ray: origin P_h + B*2^-10, direction B / r_B, tmax r_B * (1 - 2^-9): both ends are
 *     pulled in by 2^-10 of the leg, as the direct gather pulls in its receiver end.  An occlusion query answers.
 *   x_s = (lost or occluded) ? 0 : w'
 *   m_k[t] = nn == 0 ? 0 : ((double)photons_equiv * (0.5*nn)) * ((sum_s x_s) / (double)S)             the sum in sample order
 *   expected[t] = (add || k > 0) ? expected[t] + m_k[t] : m_k[t]
 * With uvrt_set_gather_faces(1) the same sum, split by f_s as uvrt_gather_direct splits it, is added into faces[f][t] under the
 * same rule, so the face-resolved bounces see the specular light as a source; with the state off `faces` is untouched.
 * Every operator one rounding, no atomics: a pure function of the arguments, whatever the capacity or the cut of a range
 * into calls.  In a room whose mirror wall is taken away, the direct gather of the mirrored lamp gives the same bits wherever
 * no sample is lost or occluded and the mirroring is exact ("the virtual lamp").
 * The call writes no variance; leaves SEED, tempPhotonMap, the source plane, links, rho and a gather batch alone; drops "the
 * last generate" like every shadow-ray call; and forgets the remembered gather, so a uvrt_gather_refine behind it is refused
 * and cannot merge into a plane that already holds specular light.  Entries outside the range are untouched.
 * UVRT_ERR_INVALID with nothing changed: no panels, flavour 2, samples outside [1, 4096] or above the capacity, T*S >= 2^31,
 * photons_equiv <= 0, add other than 0 / 1, a range outside [0, T], no scene, a null argument. */
#define UVRT_MIRROR_MAX 8
typedef struct {
    float   point[3];        /* q: any point of the plane */
    float   normal[3];       /* m: not zero; the panel reflects on the side it points to */
    float   reflectance;     /* rho in [0, 1] */
    int32_t reserved;        /* 0 */
} uvrt_mirror;               /* 32 bytes */
int uvrt_set_mirrors(uvrt_ctx* ctx, const uvrt_mirror* panels, int32_t count, const uint8_t* panel_of_tri);
int uvrt_mirror_info(uvrt_ctx* ctx, int32_t out4[4]);
int uvrt_read_mirrors(uvrt_ctx* ctx, uvrt_mirror* panels_out, uint8_t* panel_of_tri_out);
int uvrt_drop_mirrors(uvrt_ctx* ctx);
int uvrt_gather_mirror(uvrt_ctx* ctx, const uvrt_gather_params* launch, int32_t add, int32_t first_tri, int32_t tri_count);

/* ---- sensors: virtual dosimeters at points off the mesh ----
 * Every gather above answers for a triangle of the scan.  A dosimeter card taped to a wall, a radiometer head on a stand and
 * the fluence rate at a point in free air are receivers that are no triangle: a sensor is a point with either a normal (a
 * planar, one-sided receiver: irradiance) or none (a spherical receiver: fluence rate).  Everything here is additive: with no
 * sensors set every call above keeps its bits, results and call sequence.
 *
 * State.  The sensors belong to the context, not to the scene: they need no scene to be set, and uvrt_set_scene leaves them
 * and their planes alone.  With K sensors the context holds five planes f64[K], numbered as uvrt_read_sensor_plane's `which`:
 * 0 density, 1 variance, 2 dose_map, 3 max_map, 4 var_map.
 *
 * uvrt_set_sensors: count in [1, 2^24]; every position and normal finite, a planar sensor's normal not zero (a spherical
 * sensor's is not read), kind one of the two, reserved 0.  The whole input is checked before anything is changed; then it
 * replaces any earlier set and all five planes are zeroed.  uvrt_sensor_info: out4 = {count (0: none), 0, 0, 0}.
 * uvrt_read_sensors: the records as they were set; UVRT_ERR_INVALID when there are none.  uvrt_drop_sensors: drops the sensors
 * and the planes (UVRT_OK when there are none).
 *
 * uvrt_gather_sensors writes density[k] and variance[k] for k in [first, first + count), under the context's sampling mode
 * (uvrt_set_gather_sampling), flavours 0 and 1.  Sensor k has p = pos; for sample s < S = launch->samples, j = k*S + s (uint32):
 *     rng = WangHash(j ^ WangHash(seed));  xi_h, xi_m = RandomFloat(&rng) x 2
 *     UVRT_GATHER_INDEPENDENT:  u_h = xi_h, u_m = xi_m
 *     UVRT_GATHER_STRATIFIED:   u_h = fl(fl((float)s + xi_h) / (float)S);  h_k = WangHash(k ^ WangHash(seed ^ 0x9E3779B9u));
 *                               u_m = (float)((s*0x9E3779B9u + h_k) >> 8) * 2^-24
 *     o    = uvrt_generate_sweep's origin with r1 := u_h, u := u_m                              (as uvrt_gather_direct forms it)
 *     d    = p - o,  r = sqrtf((d.x*d.x + d.y*d.y) + d.z*d.z),  dir = d / r,  tmax = r * (1 - 2^-10)        (f32)
 *     D    = (double)d,  R2 = (D.x*D.x + D.y*D.y) + D.z*D.z,  R = sqrt(R2)
 *     planar:     n = (double)normal,  nn = sqrt((n.x*n.x + n.y*n.y) + n.z*n.z),  c = (n.x*D.x + n.y*D.y) + n.z*D.z
 *                 w = c < 0 ? (-c) / (nn * (R2*R) * 12.566370614359172) : 0.0
 *     spherical:  w = 1.0 / (R2 * 12.566370614359172)
 * A planar sensor is one-sided: light travelling along D arrives on the side the normal points to iff n.D < 0.  A sample with
 * r not finite or not > 0 weighs 0; a sample that weighs 0 is not traced (dir (0,1,0), tmax 0).  x_s = occluded ? 0 : w,
 *     density[k]  = (double)photons_equiv * (sum_s x_s / (double)S)
 * expected photons per square metre of a planar sensor, per square metre of cross-section of a spherical one: the unit of
 * expected[t] / area_t.  variance[k] takes the two forms of uvrt_set_gather_variance with c = (double)photons_equiv (m, q, SS
 * and v as there, variance[k] = (c*c) * v); it is written whenever S >= 2, whatever the context's variance state, and is 0 at
 * S = 1.  Every operator one rounding, the sums in sample order, no atomics: a pure function of the arguments, whatever the
 * capacity (sensors go in chunks of floor(capacity / S)) or the cut of a range into calls.
 *
 * uvrt_gather_sensors_indirect adds one diffuse bounce to density[k] of the range.  S2 = params->samples, j = k*S2 + s,
 * rng = WangHash(j ^ WangHash(seed)); (x, y) in the unit disc by uvrt_gather_indirect's bounded rejection (up to 8 rounds of
 * two draws, then x = y = 0), q = x*x + y*y, all in f64:
 *     planar:     z = sqrt(1.0 - q);  a = the axis of the smallest |n| component (x before y before z on ties);
 *                 C = cross(a, n) written out: a = x: (0.0, -n.z, n.y);  a = y: (n.z, 0.0, -n.x);  a = z: (-n.y, n.x, 0.0)
 *                 T = C / sqrt((C.x*C.x + C.y*C.y) + C.z*C.z),  B = cross(n, T) / nn  (B.x = (n.y*T.z - n.z*T.y) / nn, ...)
 *                 D.c = ((x*T.c) + (y*B.c)) + ((z/nn)*n.c)                              every sample leaves on the normal's side
 *     spherical:  g = sqrt(1.0 - q);  D = ((2.0*x)*g, (2.0*y)*g, 1.0 - 2.0*q)            Marsaglia's map: uniform on the sphere
 * dir = (float)D, origin p, tmax 1e30f; a direction that is not finite or is zero is not traced, as in uvrt_gather_indirect.
 * A closest-hit query answers h.  With n_h = cross(e1, e2) of h and nn_h = |n_h| in f64, a miss or nn_h == 0 giving 0:
 *     emitter 0:  y_s = (double)reflectance * (source[h] / (0.5*nn_h))                            the source plane
 *     emitter 1:  a = ((n_h.x*dir.x + n_h.y*dir.y) + n_h.z*dir.z) < 0 ? 0 : 1                     the face the ray arrives on
 *                 y_s = rho_a * (faces[a][h] / (0.5*nn_h)),  rho_a = use_map ? (double)rho[a][h] : (double)reflectance
 *     planar:     density[k] += (sum_s y_s) / (double)S2           the mean radiosity over cosine samples is the irradiance
 *     spherical:  density[k] += (4.0 * sum_s y_s) / (double)S2     the fluence is 4 pi times the mean radiance
 * variance[k] is left alone: it is the direct part's.
 *
 * Both tracing calls run on the context's stream behind outstanding launches, leave SEED, tempPhotonMap, expected, variance,
 * faces, source, the links, the reflectance map, the panels and the remembered gather of uvrt_gather_refine untouched, and
 * drop "the last generate" as uvrt_gather_direct does.  Mirror panels do not reach a sensor.
 *
 * uvrt_accumulate_sensors is cl/accumulate.cl's rule per sensor, in this order: dose_map += density * (double)time_step;
 * max_map = max(max_map, density); var_map += variance * ((double)time_step * (double)time_step); density = variance = 0.
 * uvrt_reset_sensors zeroes the five planes.  uvrt_read_sensor_plane / uvrt_write_sensor_plane are uvrt_read_variance /
 * uvrt_write_variance for plane `which` over [first, first + count) of [0, K]; they synchronise.  uvrt_sensor_dosage is
 * uvrt_compute_dosage's arithmetic with area = 1.0f, read back:
 *     out[i] = (float)(((double)scaled_power * map[first + i]) / (double)(1.0f * (float)photons_per_light))
 * map = dose_map (UVRT_MAP_SUM) or max_map (UVRT_MAP_MAX); it synchronises.
 *
 * UVRT_ERR_INVALID with nothing changed: a null argument; no sensors; a range outside [0, K]; K*S >= 2^31; S outside
 * [1, 4096] (S2: even, [2, 4096]) or above the capacity; photons_equiv <= 0; a non-zero reserved field; a kind or plane or
 * map number out of range; a non-finite value or a planar sensor's zero normal; a reflectance outside [0, 1] or not finite;
 * and for the two tracing calls no scene, flavour 2, emitter or use_map out of range, use_map with emitter 0 or without
 * reflectance planes (uvrt_fill_reflectance / uvrt_write_reflectance). */
enum { UVRT_SENSOR_PLANAR = 0, UVRT_SENSOR_SPHERICAL = 1 };
#define UVRT_SENSOR_MAX (1 << 24)
typedef struct {
    float   pos[3];
    float   normal[3];       /* planar: finite, not zero; the side it points to is the sensitive one.  spherical: finite, not read */
    int32_t kind;
    int32_t reserved;        /* 0 */
} uvrt_sensor;               /* 32 bytes */
typedef struct {
    float    reflectance;    /* rho in [0, 1] */
    int32_t  samples;        /* S2: even, in [2, 4096]; S2 <= capacity; K*S2 < 2^31 */
    uint32_t seed;
    int32_t  emitter;        /* 0: the source plane, 1: the face planes */
    int32_t  use_map;        /* 0 / 1: the reflectance planes in place of `reflectance`; emitter 1 only */
    int32_t  reserved;       /* 0 */
} uvrt_sensor_indirect_params;
int uvrt_set_sensors(uvrt_ctx* ctx, const uvrt_sensor* sensors, int32_t count);
int uvrt_sensor_info(uvrt_ctx* ctx, int32_t out4[4]);
int uvrt_read_sensors(uvrt_ctx* ctx, uvrt_sensor* sensors_out);
int uvrt_drop_sensors(uvrt_ctx* ctx);
int uvrt_gather_sensors(uvrt_ctx* ctx, const uvrt_gather_params* launch, int32_t first, int32_t count);
int uvrt_gather_sensors_indirect(uvrt_ctx* ctx, const uvrt_sensor_indirect_params* params, int32_t first, int32_t count);
int uvrt_accumulate_sensors(uvrt_ctx* ctx, float time_step);
int uvrt_reset_sensors(uvrt_ctx* ctx);
int uvrt_read_sensor_plane(uvrt_ctx* ctx, int32_t which, double* out, int32_t first, int32_t count);
int uvrt_write_sensor_plane(uvrt_ctx* ctx, int32_t which, const double* in, int32_t first, int32_t count);
int uvrt_sensor_dosage(uvrt_ctx* ctx, int32_t which_map, int32_t photons_per_light, float scaled_power, float* out,
                       int32_t first, int32_t count);

/* ---- batched tracing: several launches in one go, one count "plane" per launch ----
 *
 * A computation is iterations x lamps launches of generate -> extend -> accumulate (raytracer.cpp:66-88).
 * accumulate.cl:9-13 needs every launch's TOTAL per-triangle count (max), so a job that shards launches by
 * global-id range over GPUs keeps one int32[T] plane per launch, sums all planes over the ranks ONCE per
 * batch and then replays accumulate (and the host loop's Shade calls) plane by plane: the f64 maps, the dose
 * and the colours come out bit-identical to the per-launch sequence.  On one GPU the same calls trace the
 * launches of a batch in as few kernel launches as their lamps allow (launches of one lamp column share their
 * per-launch records), which keeps the persistent wavefronts supplied with rays across launch boundaries. */
typedef struct {
    float duration;              /* accumulate.cl timeStep of this launch (raytracer.cpp:84) */
    int32_t shade;               /* != 0: the host loop runs Shade after this launch (myapp.cpp:160) ... */
    int32_t which_map;           /* ... with these arguments (raytracer.cpp:96-118; UVRT_MAP_SUM / UVRT_MAP_MAX) */
    int32_t photons_per_light;
    float scaled_power, min_value;
    int32_t threshold_view;
} uvrt_replay_op;

/* generate + extend for `count` launches (<= 64), launch k from lamp lamps[3k..3k+2], all over the global
 * ids [first_gid, first_gid + n).  The SEED chain advances launch by launch exactly as `count` calls of
 * uvrt_generate would.  The deposits stay in the batch's planes until uvrt_replay_batch. */
int uvrt_trace_batch(uvrt_ctx* ctx, const float* lamps, float light_length, int32_t count,
                     int64_t first_gid, int64_t n);
/* uvrt_trace_batch for launches of either kind: launch k is a stop at launches[k].from, or a sweep from launches[k].from
 * to launches[k].to (uvrt_generate_sweep).  The SEED chain advances in logical order, by uvrt_seed_next_mode at a stop and
 * by uvrt_seed_next_sweep at a sweep; every launch has its own count plane, and fold, reduce, read, plan capture, replay and
 * uvrt_device_ptr(ctx, 5, ...) work as after uvrt_trace_batch.  Stops are traced as uvrt_trace_batch traces them (a batch
 * of stops only is that call); all sweeps of the batch share the scene's free-origin records and are traced by the
 * free-origin kernel, several planes per kernel launch.  UVRT_ERR_INVALID, with nothing changed (SEED, the batch, the launch
 * lanes): whatever uvrt_trace_batch refuses, a kind other than the two below, and a sweep under uvrt_set_seed_mode(ctx, 1)
 * or uvrt_set_flavour(ctx, 2). */
enum { UVRT_LAUNCH_STOP = 0, UVRT_LAUNCH_SWEEP = 1 };
typedef struct {
    float from[3];      /* the lamp's foot (a stop), or where the sweep starts */
    float to[3];        /* where the sweep ends; ignored for a stop */
    int32_t kind;       /* UVRT_LAUNCH_STOP / UVRT_LAUNCH_SWEEP */
    int32_t reserved;   /* 0 */
} uvrt_launch;
int uvrt_trace_batch_launches(uvrt_ctx* ctx, const uvrt_launch* launches, float light_length,
                              int32_t count, int64_t first_gid, int64_t n);
/* per launch (logical order): accumulate.cl, then Shade where ops[k].shade is set; ends the batch.
 * tri_count in [0, T]: triangles [0, tri_count) are replayed from their launches' totals exactly as a full replay would replay
 * them (folded or not, with or without dedupe and mask classes); both maps, the dose and the colours stay untouched from
 * tri_count on.  Whatever tri_count is, the batch ends and its planes are cleared entirely: the counts of the triangles from
 * tri_count on are dropped, as accumulate.cl leaves them out. */
int uvrt_replay_batch(uvrt_ctx* ctx, const uvrt_replay_op* ops, int32_t count, int32_t tri_count);
/* sum the deposit replicas of every plane into the int32[count][T] array the reduction works on */
int uvrt_fold_batch(uvrt_ctx* ctx);
/* test hook: tempPhotonMap of launch `launch` of the traced batch (folds; after a reduce: the global counts) */
int uvrt_read_batch_counts(uvrt_ctx* ctx, int32_t launch, int32_t* out, int32_t first, int32_t count);

/* ---- batched tracing: every distinct photon of a lamp is traced once ----
 * generate.cl:13 seeds work-item gid from an f32 sum, 17 gid + 1 + 13 lx + 7 ly + 11 lz + (SEED >> 15), that takes even values
 * only above 2^24 and moves by less than 131 072 from launch to launch, so the launches of ONE lamp position draw mostly the
 * same hash inputs at shifted gids: about half of the photons of 8 launches x 2 M are copies of another one (same ray, same
 * hit).  A batch therefore traces the stops of a lamp column as dedupe groups -- up to 31 launches with one bit-identical lamp,
 * in logical order: each distinct ray is traced once and its hit deposited in the plane of every launch that holds it.  The
 * planes, and everything made of them, are bit for bit what tracing every launch's rays gives.  Traced as they are: a column
 * of one launch, lamps that differ in y, sweeps, a range that ends past global id 126 322 567, a lamp coordinate of 1e7 and
 * more, and everything outside a batch (uvrt_extend).  Duplicates are looked for within the call's own global-id range, so
 * the ranks of a sharded job each dedupe their own range.
 * uvrt_set_dedupe(ctx, 0) switches it off for later batches; the default is on, or what the environment variable
 * UVRT_DEDUPE (0 / 1) says when the context is created. */
int uvrt_set_dedupe(uvrt_ctx* ctx, int32_t on);
/* Mask classes: one deposit per traced ray.  A traced ray of a dedupe group deposits its hit once per launch that holds it,
 * and a group's rays hold few distinct sets of launches.  With classes each of the group's most frequent sets of two and more
 * launches gets a count plane of its own behind the launch planes of the batch: a ray of that set deposits there once, and
 * the fold / replay adds a class plane into every launch of its set.  The per-launch totals are the same integers, so planes,
 * maps, dose and colours do not change by a bit.  The class list is found on the host from a fixed sample of the call's range
 * (a function of the lamp, the SEEDs, the range and the seed mode alone); a ray whose set has no class deposits per launch as
 * before.  Groups of 31 launches take no classes.
 * uvrt_set_dedupe_classes(ctx, max_classes): classes per group at most, 0..32; 0 deposits per launch throughout.  Takes effect
 * with the next batch; the default is uvrt_dedupe_classes_default(), or what the environment variable UVRT_DEDUPE_CLASSES says
 * when the context is created.  A value outside 0..32: UVRT_ERR_INVALID, the setting unchanged. */
int uvrt_set_dedupe_classes(uvrt_ctx* ctx, int32_t max_classes);
int uvrt_get_dedupe_classes(uvrt_ctx* ctx, int32_t* max_classes);
int32_t uvrt_dedupe_classes_default(void);
/* test hook: the atomic adds the traced rays of the last batch's dedupe groups issue if each of them hits -- one for a ray
 * that deposits in one plane (its launch's own or a class plane), one per launch for any other (waits for the batch) */
int uvrt_batch_deposits(uvrt_ctx* ctx, int64_t* out);
/* test hook: the number of non-zero int32 values in the whole allocation of the count planes of both buffer sets of the
 * context -- launch planes and class planes, used by the last batches or not.  Between batches it is 0: whatever a batch
 * deposited, its fold or replay read back and zeroed (nothing else clears a set).  UVRT_ERR_INVALID while a traced batch has
 * not been replayed.  Waits for everything the context has outstanding and copies the planes to the host. */
int uvrt_batch_residue(uvrt_ctx* ctx, int64_t* nonzero);
/* test hook, host only: the class list a batch gives the dedupe group of uvrt_dedupe_plan's arguments when it may take up to
 * max_classes classes and shares its class planes with no other group -- class_masks[0, *class_count), most frequent first,
 * room for 32 -- and, where `deposits` is not null, the group's uvrt_batch_deposits figure with that list (max_classes 0 or a
 * group of 31 launches: no classes, one deposit per occurrence). */
int uvrt_dedupe_classes(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                        int32_t seed_mode, int64_t first_gid, int64_t n, int32_t max_classes, uint32_t* class_masks,
                        int32_t* class_count, int64_t* deposits);
/* Developer knob: the instruction-issue priority (s_setprio level, 0..3) of the short kernels that run beside another launch
 * lane's persistent traversal grid -- generate, the dedupe passes, fold, replay, accumulate, Shade, reset, the per-launch
 * records.  Such a kernel's waves are the youngest on their SIMD and at level 0 issue only in the slots the traversal's waves
 * leave; a level above 0 lets them issue when they are ready.  It changes when instructions issue, never what they compute:
 * every result is bit for bit the same at every level.  The traversal kernels take no level.  Takes effect with the next
 * launch; the default is 1, or what the environment variable UVRT_HELPER_PRIO (0..3) says when the context is created.
 * A value outside 0..3: UVRT_ERR_INVALID, the level unchanged. */
int uvrt_set_helper_priority(uvrt_ctx* ctx, int32_t prio);
int uvrt_get_helper_priority(uvrt_ctx* ctx, int32_t* prio);
/* test hook: the rays the traversal kernel was given for the stops of the last traced batch (waits for the batch) */
int uvrt_batch_traced_rays(uvrt_ctx* ctx, int64_t* out);
/* test hooks, host only.  uvrt_seed_input: what work-item gid of a launch hands to the hash (generate.cl:13; the rules of
 * uvrt_set_seed_mode).  uvrt_dedupe_plan: the masks of a dedupe group of `count` launches from `lamp` over the global ids
 * [first_gid, first_gid + n), masks[k * n + i] for launch k, gid first_gid + i: 0 = another occurrence traces this ray, else
 * bit j = its hit goes to launch j's plane.  UVRT_ERR_INVALID when the launches cannot form a group (above). */
uint32_t uvrt_seed_input(int64_t gid, const float lamp[3], uint32_t seed_prev, uint32_t seed_next, int32_t seed_mode);
int uvrt_dedupe_plan(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                     int32_t seed_mode, int64_t first_gid, int64_t n, uint32_t* masks);
/* test hooks for the form of the rule the device runs: one pass per key tile instead of a search per occurrence.
 * uvrt_dedupe_plan_tiled (host only): the same group, the masks of the chunk [chunk_first, chunk_first + chunk_n) inside the
 * range, masks[k * chunk_n + i], computed tile by tile with tiles of `tile_keys` keys, in strips of tiles with carried run
 * bounds -- the functions the kernel runs, on the CPU.  They equal uvrt_dedupe_plan's for every tile width and chunk.
 * uvrt_dedupe_mark_device: the first kernel of a deduped chunk's generate alone, for that group and chunk on the context's
 * stream (waited for): every occurrence's mask as above, and the owners (non-zero masks) per launch and block of 2 048 gids
 * of the chunk, block_owner_counts[k * ceil(chunk_n / 2048) + b], as the scan pass reads them in a traced chunk (the hook
 * zeroes lane 0's counts again behind its copy, as the write pass of a traced chunk leaves them). */
int uvrt_dedupe_plan_tiled(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                           int32_t seed_mode, int64_t first_gid, int64_t n, int32_t tile_keys, int64_t chunk_first,
                           int64_t chunk_n, uint32_t* masks);
/* the same with strips of `strip_tiles` tiles (uvrt_dedupe_plan_tiled walks the device's shortest, 4): only a strip's first
 * tile searches its run bounds, the others carry them.  The masks do not depend on the strip length either. */
int uvrt_dedupe_plan_strips(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                            int32_t seed_mode, int64_t first_gid, int64_t n, int32_t tile_keys, int32_t strip_tiles,
                            int64_t chunk_first, int64_t chunk_n, uint32_t* masks);
int uvrt_dedupe_mark_device(uvrt_ctx* ctx, const float lamp[3], int32_t count, const uint32_t* seed_prev,
                            const uint32_t* seed_next, int32_t seed_mode, int64_t first_gid, int64_t n, int64_t chunk_first,
                            int64_t chunk_n, uint32_t* masks, uint32_t* block_owner_counts);
/* The period table: away from a few events -- the ends of the range, a sum that crosses a power of two, work-item 0 -- the
 * mask of an occurrence is an exact periodic function of its gid with a period of 2 to 16 gids (csrc/uvrt_dedupe.h "period
 * table").  With the table on, the host builds per interior of the group's key strata a table of launches x period deposit
 * words, the mark pass walks only the keys outside the interiors, and the write pass and the owner counts read the table for
 * the rest.  Rays, deposit words, their order and every count are bit for bit those of the general path, which still takes
 * gid 0, groups of 31 launches, short or unproven interiors and whatever 12 interiors of 384 words in all do not hold.
 * uvrt_set_dedupe_periodic(ctx, on): takes effect with the next batch; the default is on (DESIGN.md section 15 has the
 * measurement), or what the environment variable UVRT_DEDUPE_PERIODIC (0 / 1) says when the context is created. */
int uvrt_set_dedupe_periodic(uvrt_ctx* ctx, int32_t on);
int uvrt_get_dedupe_periodic(uvrt_ctx* ctx, int32_t* on);
/* test hook, host only: uvrt_dedupe_plan_tiled's chunk through the period table -- the functions the batch and its kernels
 * run, on the CPU: masks[k * chunk_n + i], the owners per launch and block of 2 048 gids as uvrt_dedupe_mark_device lays them
 * out (the interiors' in closed form from the table), and *from_table = the occurrences whose mask came from the table. */
int uvrt_dedupe_plan_periodic(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                              int32_t seed_mode, int64_t first_gid, int64_t n, int64_t chunk_first, int64_t chunk_n,
                              uint32_t* masks, uint32_t* block_owner_counts, int64_t* from_table);
/* test hook: the three generate kernels of a deduped chunk alone, for that group and chunk with the context's settings (mask
 * classes, period table), on the context's stream (waited for): the compacted rays (16 bytes each) and deposit words in
 * (launch, gid) order, room for count x chunk_n of each; *total = rays written, *deposits = the atomics they stand for. */
int uvrt_dedupe_generate_device(uvrt_ctx* ctx, const float lamp[3], float light_length, int32_t count, const uint32_t* seed_prev,
                                const uint32_t* seed_next, int32_t seed_mode, int64_t first_gid, int64_t n, int64_t chunk_first,
                                int64_t chunk_n, float* rays, uint32_t* words, uint32_t* total, uint32_t* deposits);

/* ---- the one collective of a sharded computation (RCCL over xGMI; librccl is opened on first use) ----
 * One process per GPU: rank 0 calls uvrt_comm_unique_id and hands the 128 bytes to every rank (any
 * out-of-band channel), every rank calls uvrt_comm_init_rank; then per batch uvrt_trace_batch (its own
 * global-id range) -> uvrt_reduce_batch (int32 SUM all-reduce of the planes on the context's stream) ->
 * uvrt_replay_batch.  One process driving several GPUs: uvrt_comm_init_all over one context per device and
 * uvrt_reduce_batch_group.  uvrt_reduce_batch_group without communicators sums contexts that share ONE
 * device (rehearsals and tests of the sharded path on a single-GPU box). */
/* 1 when librccl opens and every entry point used here resolves, else 0 (text in uvrt_last_error): a LOCAL
 * precondition.  uvrt_comm_init_rank is itself a collective (ncclCommInitRank): ranks agree on this flag over their
 * out-of-band channel first, so that a rank without RCCL cannot leave the others waiting inside the init. */
int uvrt_comm_available(void);
int uvrt_comm_unique_id(void* id128);
int uvrt_comm_init_rank(uvrt_ctx* ctx, const void* id128, int32_t rank, int32_t world);
int uvrt_comm_init_all(uvrt_ctx** ctxs, int32_t n);
int uvrt_comm_destroy(uvrt_ctx* ctx);
/* what the context's communicator is: out4 = { world given at init (0: none), rank, ncclCommCount of the native
 * communicator (what RCCL itself spans; 0: none), compute units the launch lanes leave to the collective } */
int uvrt_comm_info(uvrt_ctx* ctx, int32_t out4[4]);
int uvrt_reduce_batch(uvrt_ctx* ctx);
int uvrt_reduce_batch_group(uvrt_ctx** ctxs, int32_t n);

/* ---- duration planning: the least total exposure that reaches a minimum dose ----
 * The dose is linear in the lamp durations and the photon counts do not depend on them.  A planning computation
 * traces I iterations over P candidate positions and captures, per position p and triangle t, the photons of p that
 * hit t summed over the iterations: E[p][t] (exact uint32).  With N = I x photonsPerLight, s = lightIntensity x 0.1f
 * and den_t = area_t x (float)N (f32, as computeDosage forms it), the model dose is
 *     D_t(d) = s x sum_p E[p][t] x d_p / den_t        (f64)
 * and uvrt_plan_solve finds durations d >= 0 of least sum with D_t(d) >= min_dose x (1 + margin) on every REQUIRED
 * triangle: one that passes the caller's mask and has sum_p E[p][t] >= min_photons (> 0).  Rows it leaves out are
 * reported as unreachable (no photon; or zero area), unresolved (0 < photons < min_photons) and masked out.  The solver
 * works by cutting planes: the GPU evaluates every row under the current durations, the host picks the most violated
 * rows from those values and the GPU gathers them; the host solves the LP restricted to the rows gathered so far (a
 * warm-started simplex) and repeats until the certified gap is <= rel_gap or the round cap is reached.  The durations it
 * returns are feasible in f64 after their rounding to f32 (and print back to themselves as "%.8g"), and a dual vector
 * y >= 0 certifies LB = sum_t y_t / max_p (A^T y)_p <= OPT.  Calling sequence: uvrt_plan_begin -> per batch uvrt_trace_batch
 * (-> uvrt_reduce_batch*) -> uvrt_plan_capture_batch -> uvrt_replay_batch -> ... -> uvrt_plan_solve.
 * uvrt_set_scene drops the planning state.  A "position" is any launch whose count plane is a column of E: the sweeps of
 * uvrt_trace_batch_launches are captured like stops, and uvrt_plan_solve_bounded (below) plans with columns whose
 * duration is given in advance -- a route that radiates while it drives. */
enum { UVRT_PLAN_CONVERGED = 0, UVRT_PLAN_ITERATION_CAP = 1 };
typedef struct {
    float min_dose;                 /* m, mJ/cm^2 (the route's minimale_dosis); <= 0: every duration 0 */
    float scaled_power;             /* s = lightIntensity * 0.1f (Shade's factor) */
    int64_t photons_per_position;   /* N = iterations * photonsPerLight, Shade's divisor; <= 2^32 - 1 */
    int32_t min_photons;            /* a triangle with fewer captured photons is "unresolved", not required */
    int32_t max_iterations;         /* cap on the cutting-plane rounds (<= 0: 200) */
    double margin;                  /* relative safety factor on m (1e-6 by default) */
    double rel_gap;                 /* stop at (sum d - LB) / sum d <= rel_gap */
    const uint8_t* mask;            /* uint8[T], 0 = not required; NULL: every triangle may be */
    int32_t reserved[2];            /* 0 */
} uvrt_plan_params;
typedef struct {
    int32_t status;                 /* UVRT_PLAN_CONVERGED (gap <= rel_gap) or UVRT_PLAN_ITERATION_CAP (still feasible) */
    int32_t iterations;             /* cutting-plane rounds */
    int32_t positions;              /* P */
    int32_t used_positions;         /* durations > 0 */
    int32_t required, unreachable, unresolved, masked_out;     /* triangle counts */
    double area_required, area_unreachable, area_unresolved, area_masked_out;
    double total_duration;          /* sum d (f64 over the f32 durations) */
    double lower_bound;             /* LB <= OPT <= total_duration */
    double gap;                     /* (total_duration - LB) / total_duration (0 when both are 0) */
    double min_dose_ratio;          /* min over the required triangles of D_t(d) / m (+inf for an empty set) */
} uvrt_plan_report;
/* allocate and zero E for P in [1, 256] positions (P x T < 2^32); drops an earlier plan.  E (P x T x 4 bytes) stays
 * allocated until uvrt_plan_end, uvrt_set_scene or uvrt_destroy. */
int uvrt_plan_begin(uvrt_ctx* ctx, int32_t positions);
/* add the count planes of the traced batch to E: launch k (logical order) goes to row position_of_launch[k].  Folds the
 * batch first if needed; call it after uvrt_trace_batch (and any uvrt_reduce_batch*: it then captures the global counts)
 * and before uvrt_replay_batch, which computes exactly what it would have without the capture. */
int uvrt_plan_capture_batch(uvrt_ctx* ctx, const int32_t* position_of_launch, int32_t count);
/* solve; durations_out: float[P]; synchronises.  UVRT_ERR_INVALID also when a captured count overflowed uint32. */
int uvrt_plan_solve(uvrt_ctx* ctx, const uvrt_plan_params* params, float* durations_out, uvrt_plan_report* report);
/* D_t(d) as f32 for any durations float[P], with s and N of the last uvrt_plan_solve; synchronises */
int uvrt_plan_model_dose(uvrt_ctx* ctx, const float* durations, float* out, int32_t first, int32_t count);
/* test hooks: row `position` of E; the required set of the last solve (1 = required; after a bounded solve: active or
 * met by the bounds); both synchronise */
int uvrt_plan_read_exposure(uvrt_ctx* ctx, int32_t position, uint32_t* out, int32_t first, int32_t count);
int uvrt_plan_read_required(uvrt_ctx* ctx, uint8_t* out, int32_t first, int32_t count);
/* test hook: host values into E[position][first .. first + count) of a COUNTS plan, so that a test can plan on a matrix no
 * trace gives (row sums past 2^32, competing classes, ties).  It counts as a capture (a solve does not refuse with "nothing
 * captured") and leaves the per-position ray bookkeeping of uvrt_plan_capture_batch and the overflow flag as they are;
 * synchronises.  UVRT_ERR_INVALID with nothing changed: an expected plan (uvrt_write_expected + uvrt_plan_capture_expected
 * carry hand-written planes there), no plan, a position outside [0, P), a range outside [0, T), a null pointer. */
int uvrt_plan_write_exposure(uvrt_ctx* ctx, int32_t position, const uint32_t* in, int32_t first, int32_t count);
int uvrt_plan_end(uvrt_ctx* ctx);
/* ---- bounded solve: columns with a value given in advance (a route that radiates while it drives) ----
 * d_p >= lower[p] on every column, and a FIXED column is no variable at all: d_p = lower[p].  With x = lower + e the
 * solver minimises sum e over the free columns subject to sum_{free p} E[p][t] r_t e_p >= rho_t = 1 - base_t on the
 * ACTIVE rows, r_t = s / (den_t m'), base_t = (sum_p E[p][t] lower[p]) r_t (f64, ascending p); divided by rho_t that is
 * the homogeneous covering LP of uvrt_plan_solve with the row scale r_t / rho_t (rho_t clamped from below to 1e-9:
 * clamping upward only tightens the LP).  Every triangle gets one class, tested in this order:
 *   3 masked out; 1 unreachable (no photon of any column, or no area); 2 unresolved (fewer than min_photons);
 *   4 met by the bounds (base_t >= 1); 5 short (below m' at `lower` and no free column reaches it: left out, reported);
 *   0 active.  `required` of the report = classes 0 and 4 (what uvrt_plan_read_required marks); short rows are not.
 * With min_dose <= 0 every class 0 / 4 / 5 row is class 4 and durations_out = lower.
 * Result: a fixed column returns lower[p] bit for bit, so does a free column whose e_p is 0; otherwise the smallest
 * uvrt_plan_round_trip_up value >= lower[p] + e_p.  The final check is in x-space, in f64, over the required rows:
 * (sum_p E[p][t] out_p) r_t >= 1, and min_dose_ratio comes from it.  Report: positions = P, used_positions = columns
 * with out > 0, total_duration = sum out, lower_bound = lower_total + the residual LP's certified bound,
 * gap = (total - lower_bound) / (total - lower_total) (0 when that denominator is 0).
 * bounds == NULL, or all-zero `lower` without a fixed column, is uvrt_plan_solve bit for bit (classes 0-3).
 * UVRT_ERR_INVALID, nothing changed: a negative, NaN or infinite lower[p], and whatever uvrt_plan_solve refuses. */
typedef struct {
    const float*   lower;   /* float[P]: d_p >= lower[p]; finite, >= 0.  NULL: all 0 */
    const uint8_t* fixed;   /* uint8[P]: != 0 -> d_p = lower[p] exactly, not a variable.  NULL: none */
    int32_t reserved[2];    /* 0 */
} uvrt_plan_bounds;
typedef struct {
    int32_t fixed_columns, free_columns;
    int32_t met_by_lower;   /* rows that D_t(lower) already brings to m' */
    int32_t short_rows;     /* rows below m' at `lower` that no free column reaches: left out, reported */
    double  area_met_by_lower, area_short;
    double  lower_total;    /* sum of lower (f64 over the f32 values) */
    int32_t reserved[2];
} uvrt_plan_bounds_report;
int uvrt_plan_solve_bounded(uvrt_ctx* ctx, const uvrt_plan_params* params, const uvrt_plan_bounds* bounds,
                            float* durations_out, uvrt_plan_report* report, uvrt_plan_bounds_report* bounds_report /* may be NULL */);
/* test hook: the class of every triangle in the last solve (0-3 after uvrt_plan_solve); synchronises */
int uvrt_plan_read_classes(uvrt_ctx* ctx, uint8_t* out, int32_t first, int32_t count);
/* ---- planning from the direct gather: an exposure matrix of expected values ----
 * A plan is of one kind, fixed when it begins: COUNTS (uvrt_plan_begin, E[p][t] uint32 photon counts) or EXPECTED
 * (uvrt_plan_begin_expected, X[p][t] f64: the expected tempPhotonMap entries the direct gather writes, so the triangles no
 * photon reaches get a row too).  uvrt_plan_solve, uvrt_plan_solve_bounded, uvrt_plan_model_dose, uvrt_plan_read_required,
 * uvrt_plan_read_classes and uvrt_plan_end work on either kind: for an expected plan every formula above holds with X[p][t]
 * in place of (double)E[p][t].  The row sum that classes a triangle, sum_p X[p][t], and the sum over the free columns are
 * f64 sums in ascending p: "unreachable" when the sum is 0 (or no area), "unresolved" when it is < (double)min_photons,
 * "short" when the free-column sum is 0; the best position of a row is the one with the largest X, lowest index on ties.
 * Calling sequence: uvrt_plan_begin_expected -> per launch uvrt_gather_direct -> uvrt_plan_capture_expected(column) ->
 * uvrt_accumulate_expected -> ... -> uvrt_plan_solve*.  The caller owns the bookkeeping: the photons_equiv of the planes
 * captured into one column must sum to photons_per_position of the solve.  The plan is as good as the estimator: see
 * DESIGN.md 12 for the scatter of a row at S samples.
 * uvrt_plan_begin_expected: uvrt_plan_begin with X as double[P][T], zeroed; the same limits; drops a plan of either kind. */
int uvrt_plan_begin_expected(uvrt_ctx* ctx, int32_t positions);
/* X[position][t] += expected[t] for every t (one f64 addition per entry, no atomics) on the context's stream behind all
 * outstanding work; the expected plane stays as it is, so the uvrt_accumulate_expected that follows computes what it would
 * have without the capture.  A sum that is not finite or is negative raises a flag on the device (the analogue of the
 * uint32 overflow flag): uvrt_plan_solve* then returns UVRT_ERR_INVALID. */
int uvrt_plan_capture_expected(uvrt_ctx* ctx, int32_t position);
/* test hook: row `position` of X; synchronises */
int uvrt_plan_read_exposure_expected(uvrt_ctx* ctx, int32_t position, double* out, int32_t first, int32_t count);
/* UVRT_ERR_INVALID with nothing changed: uvrt_plan_capture_batch / uvrt_plan_read_exposure on an expected plan,
 * uvrt_plan_capture_expected / uvrt_plan_read_exposure_expected on a counts plan or without a plan, a position outside
 * [0, P), a null pointer. */
/* ---- planning for a lower confidence bound: an exposure matrix with its variance ----
 * The solver guarantees the minimum dose for the ESTIMATED exposure; an estimate scatters round the truth, so about half the
 * rows that bind a plan sit below the minimum in reality.  An expected plan may carry V[p][t], the variance of X[p][t]:
 * uvrt_plan_begin_expected_variance is uvrt_plan_begin_expected with V as double[P][T], zeroed, beside X (the same limits;
 * drops a plan of either kind).  On such a plan uvrt_plan_capture_expected also does V[position][t] += variance[t] (launches
 * of different seeds are independent, so their variances add as their estimates do; a sum that is not finite or is negative
 * raises the same flag); on a plan without V it is the call above.  Calling sequence: uvrt_set_gather_variance(1) ->
 * uvrt_plan_begin_expected_variance -> per launch uvrt_gather_direct -> uvrt_plan_capture_expected ->
 * uvrt_accumulate_expected -> ... -> uvrt_plan_lower_confidence(z) -> uvrt_plan_solve*.
 * uvrt_plan_lower_confidence, once per plan after the captures: for every element, in place,
 *     lo = X - z*sqrt(V);  X = lo > 0 ? lo : 0                      (one f64 rounding per operator)
 * z finite and >= 0; z = 0 leaves every bit of X as it was.  Afterwards every solve, model-dose, class and required call works
 * on the bound unchanged -- one solver -- and uvrt_plan_capture_expected on this plan and a second
 * uvrt_plan_lower_confidence return UVRT_ERR_INVALID with nothing changed.
 * Why the bound is taken per element: for durations d >= 0, sum_p z sigma_p d_p >= z * sqrt(sum_p sigma_p^2 d_p^2), so the
 * row sum of the bounds is at least as cautious as the estimate minus z standard errors of the row's own dose, for every
 * duration vector; and the problem stays the same LP (the row's own standard error would make it a second-order cone).
 * uvrt_plan_read_exposure_variance: test hook, row `position` of V; synchronises.
 * UVRT_ERR_INVALID with nothing changed: either call on a plan without V or without a plan, z negative or not finite, a
 * position outside [0, P), a null pointer. */
int uvrt_plan_begin_expected_variance(uvrt_ctx* ctx, int32_t positions);
int uvrt_plan_read_exposure_variance(uvrt_ctx* ctx, int32_t position, double* out, int32_t first, int32_t count);
int uvrt_plan_lower_confidence(uvrt_ctx* ctx, double z);
/* the smallest float >= v that "%.8g" (SaveRoute) prints back to itself through strtof (LoadRoute): how the solver rounds
 * the durations it returns.  Host only, no GPU needed. */
float uvrt_plan_round_trip_up(float v);

/* ---- tuning knobs (results never depend on them) ---- */
/* bits of the ray-coherence key used to order rays before extend; 0 = trace in gid order
 * (default), -1 = choose from n (about one wavefront of rays per key). */
int uvrt_set_sort_bits(uvrt_ctx* ctx, int32_t bits);
/* record (dist, triID) per ray in gid order during extend (the reference updates rays in
 * place, extend.cl:90-92); off by default, needed by uvrt_read_rays. */
int uvrt_set_record_hits(uvrt_ctx* ctx, int32_t on);
/* arithmetic flavour of extend (cl/extend.cl:6-38):
 *   0 (default) = the canonical strict flavour of SURVEY.md 8c: every operator one IEEE rounding in source order,
 *     correctly rounded divisions -- bit-exact against a CPU restatement unconditionally;
 *   1 = "ocl-amd": IntersectTri's cross()/dot() in the fused multiply-add forms ROCm's OpenCL device library gives the
 *     reference's extend.cl on gfx950 (strict build) -- results equal that kernel's, run
 *     live on the same GPU, bit for bit; slab test, traversal and deposit as flavour 0;
 *   2 = "shipped flags" (OPT-IN): the arithmetic the reference's OWN clBuildProgram options (-cl-fast-relaxed-math
 *     -cl-mad-enable -cl-single-precision-constant, template/template.cpp:1192) make of extend.cl on gfx950, read
 *     off the disassembly of that build: IntersectAABB's t = (b - o) * v_rcp_f32(d) (one multiply by the hardware's
 *     approximate reciprocal instead of a division, cl/extend.cl:31-35), IntersectTri as flavour 1 with
 *     f = v_rcp_f32(a) (extend.cl:17).  (dist bits, triID, counts) equal that kernel's bit for bit; against
 *     flavours 0 / 1 a few rays per million land on a neighbouring triangle (the dose stays within 1e-4).  v_rcp_f32
 *     is specific to the GPU generation: a CPU restatement reproduces this flavour only with the instruction's table
 *     read from the device.  Rays whose direction
 *     has all three components zero or NaN are outside this flavour's parity domain. */
int uvrt_set_flavour(uvrt_ctx* ctx, int32_t flavour);
/* OPT-IN 4-wide traversal: uvrt_extend walks a one-level collapse of the caller's BVH
 * (a node holds its grandchildren's boxes) -- about half the loop trips per ray, the same box and triangle
 * arithmetic, but NOT the reference's visit order: `dist` and `triID` equal the default kernel's except on
 * rays where two accepted hits tie exactly in t or a box is culled by an almost equally distant earlier hit
 * (extend.cl:25,66-76 make those order-dependent; none in 25 M rays on the test room).  Off by default: the
 * default walk is bit-exact unconditionally.  uvrt_trace_batch always uses the default walk. */
int uvrt_set_wide_bvh(uvrt_ctx* ctx, int32_t on);
/* Which node-pair records the traversal serves from LDS: 1 (default) = the 175 records the lamp's photons
 * visit most, found on the device from a sample of the launch's own rays the first time a lamp position is
 * seen (62-70 % of all inner-node visits on the test room); 0 = the first levels of the tree in breadth-first order
 * (31-40 %).  Only the order of records in memory changes; results never depend on it. */
int uvrt_set_hot_records(uvrt_ctx* ctx, int32_t mode);
/* Renumber the node-pair records of the default extend kernel: record i (breadth-first index of the
 * inner node, as uvrt_set_scene lays them out) moves to perm[i]; the first 175 records of the new
 * numbering are served from LDS.  Results do not depend on it.  NULL restores the breadth-first
 * order.  Reset by uvrt_set_scene. */
int uvrt_set_record_perm(uvrt_ctx* ctx, const uint32_t* perm, int32_t n);
/* test hook: the renumbering the launch of the last uvrt_generate uses (the caller's own, the automatic hot-record
 * one, or the identity): out[i] = index of breadth-first record i, n = number of inner nodes; synchronises. */
int uvrt_read_record_perm(uvrt_ctx* ctx, uint32_t* out, int32_t n);

/* Launch pipelining (on by default): consecutive launches (generate, extend, accumulate and the Shade
 * that follows) alternate between the context's stream and an internal second stream with their own
 * ray / count buffers, so the next launch starts in the wave slots the previous one frees while its
 * last rays finish.  The per-triangle maps are still updated in launch order and every other entry
 * point first orders the context's stream after all outstanding work, so callers see the in-order
 * behaviour of the reference's single command queue.  0 = everything on the one stream.  (The
 * tempPhotonMap pointer of uvrt_device_ptr(ctx, 2, ...) alternates with the launch lane: callers
 * that cache it across launches must switch the pipelining off.) */
int uvrt_set_pipeline(uvrt_ctx* ctx, int32_t on);

/* extend kernel knobs (developer / A-B; every setting is bit-exact): 0 = default; 400-499 = leaf period /
 * LDS top cache code + 10 * grid code with refill at 16 idle lanes; 500-599 = the same with IEEE divisions
 * everywhere; 600-1299 = like 400-499 with the refill threshold 8 / 24 / 4 / 32 / 40 / 48 / 56 idle lanes.  See DESIGN.md 4. */
int uvrt_set_variant(uvrt_ctx* ctx, int32_t variant);

/* ---- test / interop hooks ---- */
/* the rays of the last generate (+ extend, if hits were recorded) in the reference's 32-byte
 * Ray layout and gid order; synchronises. */
int uvrt_read_rays(uvrt_ctx* ctx, void* rays32, int64_t first, int64_t count);
/* test hook: replace the rays of the "last generate" by n host records in the reference's 32-byte
 * Ray layout (dir, orig; dist/triID ignored).  All records must share orig.x and orig.z (rays of
 * one lamp, generate.cl:16; uvrt_write_free_rays takes any origins).  SEED is untouched.  Lets tests feed adversarial rays (zero
 * direction components, origins on box planes) straight into uvrt_extend. */
int uvrt_write_rays(uvrt_ctx* ctx, const void* rays32, int64_t n);
int uvrt_read_counts(uvrt_ctx* ctx, int32_t* out, int32_t first, int32_t count);
int uvrt_read_photon_map(uvrt_ctx* ctx, int32_t which_map, double* out, int32_t first,
                         int32_t count);
/* raw device pointers of the per-triangle arrays, for zero-copy wrapping (e.g. as torch
 * tensors handed to an RCCL collective).  which: 0 photonMap f64[T], 1 maxPhotonMap f64[T],
 * 2 tempPhotonMap i32[T], 3 dosageMap f32[T], 4 colour f32[9T], 5 the folded planes i32[launches][T] of the
 * traced batch (for a caller that brings its own collective; uvrt_reduce_batch is the native one), 6 the direct gather's
 * expected plane f64[T], 7 its variance plane f64[T], 8 the one-bounce gather's source plane f64[T].
 * The call is also the ordering point for external work on these arrays: it orders the context's
 * stream after every outstanding launch (with launch pipelining some sit on the library's second
 * stream) and makes the library's next work on the arrays wait for whatever the caller enqueues on
 * the context's stream before its next uvrt call.  Call it before EVERY external use, not once. */
int uvrt_device_ptr(uvrt_ctx* ctx, int32_t which, void** ptr, int64_t* bytes);
/* copy one of those arrays to (to_ctx = 0) or from (to_ctx = 1) an external device buffer of the
 * same size, on the context's stream (staging for collectives when zero-copy wrapping is not
 * available). */
int uvrt_copy_device(uvrt_ctx* ctx, int32_t which, void* ext_dev_ptr, int32_t to_ctx);
/* time in ms the device spent in the extend kernels since the last call (HIP events on the
 * context's stream), and the number of extend launches; synchronises. */
int uvrt_extend_time_ms(uvrt_ctx* ctx, double* ms, int64_t* launches);
int uvrt_set_timing(uvrt_ctx* ctx, int32_t on);
/* measurement hook: the shader clock UNDER LOAD.  _start enqueues a one-wave kernel on a stream of its own that reads the
 * shader-clock counter (s_memtime) and the constant 100 MHz counter (s_memrealtime) `microseconds` apart, beside whatever the
 * context's streams are doing; _read waits for it and returns ticks ratio x 100 MHz.  bench.py prices the issue-rate peaks of its
 * roofline with the clock measured during its own steps instead of the nominal 2.4 GHz. */
int uvrt_clock_probe_start(uvrt_ctx* ctx, int32_t microseconds);
int uvrt_clock_probe_read(uvrt_ctx* ctx, double* shader_mhz);
/* compute units of the context's device (the persistent extend grid is 8 workgroups per CU) */
int uvrt_device_cus(uvrt_ctx* ctx);
/* HIP devices visible to the process (0 when there is none) */
int uvrt_device_count(void);

#ifdef __cplusplus
}
#endif
#endif

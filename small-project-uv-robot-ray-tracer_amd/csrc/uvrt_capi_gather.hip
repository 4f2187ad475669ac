// uvrt_capi_gather.hip -- shadow rays and the per-triangle direct gather (include/uvrt.h "shadow rays and the direct gather"):
// uvrt_occluded, uvrt_set_gather_sampling, uvrt_get_gather_sampling, uvrt_set_gather_variance, uvrt_get_gather_variance,
// uvrt_gather_direct, uvrt_accumulate_expected, uvrt_read_expected, uvrt_write_expected, uvrt_read_variance,
// uvrt_write_variance, uvrt_set_gather_faces, uvrt_get_gather_faces, uvrt_read_gather_faces, uvrt_write_gather_faces
// (uvrt_occlude.hip's kernels); uvrt_gather_refine, uvrt_read_gather_extra, uvrt_refine_counts (uvrt_refine.hip's)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

int ensure_expected(uvrt_ctx* c)
{
    return c->derived.expected.ensure((size_t)c->T * 8, true, c->stream);      // (nothing to do once it is there)
}

int ensure_variance(uvrt_ctx* c)
{
    return c->derived.variance.ensure((size_t)c->T * 8, true, c->stream);
}

int ensure_faces(uvrt_ctx* c)
{
    return c->derived.faces.ensure((size_t)c->T * 16, true, c->stream);
}

// the gather's per-triangle records {v0, e1, e2} in tris64 order, made from the scene's leaf triangles on first use
int ensure_gather_tris(uvrt_ctx* c)
{
    if (c->derived.g_tris_valid) return UVRT_OK;
    if (int rc = c->derived.g_tris.ensure((size_t)c->T * 48, true, c->stream)) return rc;
    launch_gather_tris(c->ltris.as<LeafTri>(), c->derived.g_tris.as<float4>(), c->T, c->stream);
    HIP_TRY(hipGetLastError());
    c->derived.g_tris_valid = true;
    return UVRT_OK;
}

// the arguments uvrt_gather_refine and uvrt_refine_counts share; `who` names the call in the message
static int check_refine_params(uvrt_ctx* c, const uvrt_refine_params* prm, const char* who)
{
    if (!(prm->rel_error > 0.0) || !std::isfinite(prm->rel_error))
        return fail(UVRT_ERR_INVALID, "%s: rel_error must be finite and > 0", who);
    if (!(prm->min_expected >= 0.0) || !std::isfinite(prm->min_expected))
        return fail(UVRT_ERR_INVALID, "%s: min_expected must be finite and >= 0", who);
    const int32_t M = prm->max_extra;
    if (M < 2 || M > 4096 || (M & (M - 1)) != 0)
        return fail(UVRT_ERR_INVALID, "%s: max_extra = %d must be a power of two in [2, 4096]", who, M);
    if ((int64_t)c->T * M >= ((int64_t)1 << 31))
        return fail(UVRT_ERR_INVALID, "%s: %d triangles x %d samples do not fit 2^31 sample numbers", who, c->T, M);
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return fail(UVRT_ERR_INVALID, "%s: reserved fields must be 0", who);
    return UVRT_OK;
}

// the refine's n_t plane, offsets and block sums, sized for the scene
static int ensure_refine_buffers(uvrt_ctx* c)
{
    if (int rc = c->derived.g_extra.ensure((size_t)c->T * 4, true, c->stream)) return rc;
    if (int rc = c->g_offs.ensure(((size_t)c->T + 1) * 4, false, c->stream)) return rc;
    return c->g_scan.ensure(((size_t)c->T / 1024 + 1) * 4, false, c->stream);
}

// Everything a shadow-ray launch works on, on the context's stream behind all outstanding work: lane 0's ray buffer, the
// scene's free records, every ray's {orig.x, orig.z}, tmax and answer.  The rays of "the last generate" are gone after it; the
// launch lane of the last generate stays the current one, so its deposits (tempPhotonMap) are still what uvrt_accumulate,
// uvrt_read_counts and uvrt_device_ptr see.
int begin_shadow_launch(uvrt_ctx* c)
{
    if (int rc = join_all(c)) return rc;
    c->last = {};                           // lane 0's rays are about to be overwritten
    if (int rc = ensure_free_records(c)) return rc;
    const size_t cap = (size_t)std::max<int64_t>(c->capacity, 1);
    if (int rc = c->g_oxz.ensure(cap * 8, false, c->stream)) return rc;
    if (int rc = c->g_tmax.ensure(cap * 4, false, c->stream)) return rc;
    if (int rc = c->g_occ.ensure(cap, false, c->stream)) return rc;
    return UVRT_OK;
}

// k_occlude_free over the first n rays of lane 0 (rays, oxz, g_tmax -> g_occ) on the context's stream
int trace_shadow_rays(uvrt_ctx* c, int64_t n, const char* who)
{
    OccludeParams op;
    fill_query_launch(c, op, n);
    op.occluded = c->g_occ.as<uint8_t>();
    return timed_launch(c, c->stream, who, "the shadow-ray launch",
                        [&] { return launch_occlude_free(op, variant_per_cu(c->variant, 8), c->stream); });
}

int upload_query_rays(uvrt_ctx* c, const void* rays32, int64_t n, int (*begin)(uvrt_ctx*))
{
    std::vector<float> packed, oxz, tmax;
    unpack_rays((const HostRay*)rays32, n, packed, &oxz, &tmax);
    if (int rc = begin(c)) return rc;
    HIP_TRY(hipMemcpyAsync(c->lanes[0].rays.p, packed.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->g_oxz.p, oxz.data(), (size_t)n * 8, hipMemcpyHostToDevice, c->stream));
    HIP_TRY(hipMemcpyAsync(c->g_tmax.p, tmax.data(), (size_t)n * 4, hipMemcpyHostToDevice, c->stream));
    return UVRT_OK;
}

}  // namespace uvrt_impl

extern "C" {

int uvrt_occluded(uvrt_ctx* c, const void* rays32, int64_t n, uint8_t* out)
{
    if (!c || !rays32 || !out) return fail(UVRT_ERR_INVALID, "uvrt_occluded: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_occluded: no scene");
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "uvrt_occluded: shadow rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", c->flavour);
    if (n < 0 || n > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_occluded: n = %lld exceeds the ray capacity %lld (uvrt_resize_rays)", (long long)n,
                    (long long)c->capacity);
    if (n == 0) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    if (int rc = upload_query_rays(c, rays32, n, begin_shadow_launch)) return rc;
    if (int rc = trace_shadow_rays(c, n, "uvrt_occluded")) return rc;
    return copy_sync(c, out, c->g_occ.p, (size_t)n, hipMemcpyDeviceToHost);
}

int uvrt_set_gather_sampling(uvrt_ctx* c, int32_t mode)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_set_gather_sampling: null context");
    if (mode != UVRT_GATHER_INDEPENDENT && mode != UVRT_GATHER_STRATIFIED)
        return fail(UVRT_ERR_INVALID, "uvrt_set_gather_sampling: mode must be 0 (independent) or 1 (stratified), not %d", mode);
    c->gather_sampling = mode;
    return UVRT_OK;
}

int uvrt_get_gather_sampling(uvrt_ctx* c, int32_t* mode)
{
    if (!c || !mode) return fail(UVRT_ERR_INVALID, "uvrt_get_gather_sampling: null argument");
    *mode = c->gather_sampling;
    return UVRT_OK;
}

int uvrt_set_gather_variance(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_set_gather_variance: null context");
    if (on != 0 && on != 1) return fail(UVRT_ERR_INVALID, "uvrt_set_gather_variance: on must be 0 or 1, not %d", on);
    c->gather_variance = on;
    return UVRT_OK;
}

int uvrt_get_gather_variance(uvrt_ctx* c, int32_t* on)
{
    if (!c || !on) return fail(UVRT_ERR_INVALID, "uvrt_get_gather_variance: null argument");
    *on = c->gather_variance;
    return UVRT_OK;
}

int uvrt_set_gather_faces(uvrt_ctx* c, int32_t on)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_set_gather_faces: null context");
    if (on != 0 && on != 1) return fail(UVRT_ERR_INVALID, "uvrt_set_gather_faces: on must be 0 or 1, not %d", on);
    c->gather_faces = on;
    return UVRT_OK;
}

int uvrt_get_gather_faces(uvrt_ctx* c, int32_t* on)
{
    if (!c || !on) return fail(UVRT_ERR_INVALID, "uvrt_get_gather_faces: null argument");
    *on = c->gather_faces;
    return UVRT_OK;
}

int uvrt_gather_direct(uvrt_ctx* c, const uvrt_gather_params* prm, int32_t first_tri, int32_t tri_count)
{
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: no scene");
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: shadow rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", c->flavour);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: triangles [%d, +%d) outside [0, %d]", first_tri, tri_count, c->T);
    const int32_t S = prm->samples;
    if (S < 1 || S > 4096) return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: samples = %d must be in [1, 4096]", S);
    const bool var = c->gather_variance != 0, sided = c->gather_faces != 0;
    if (var && S < 2)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: the variance plane needs samples >= 2 (uvrt_set_gather_variance), not %d", S);
    if ((int64_t)S > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: samples = %d exceed the ray capacity %lld (uvrt_resize_rays)", S, (long long)c->capacity);
    if ((int64_t)c->T * S >= ((int64_t)1 << 31))
        return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: %d triangles x %d samples do not fit 2^31 sample numbers", c->T, S);
    if (prm->photons_equiv <= 0) return fail(UVRT_ERR_INVALID, "uvrt_gather_direct: photons_equiv must be > 0");
    if (int rc = set_device(c)) return rc;
    c->derived.gather_memo = {};                    // remembered again below, when this call has written both planes
    if (int rc = begin_shadow_launch(c)) return rc;
    const size_t cap = (size_t)c->capacity;
    if (int rc = c->g_w.ensure(cap * 8, false, c->stream)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    if (var)
        if (int rc = ensure_variance(c)) return rc;
    if (sided) {
        if (int rc = c->g_face.ensure(cap, false, c->stream)) return rc;
        if (int rc = ensure_faces(c)) return rc;
    }
    if (int rc = ensure_gather_tris(c)) return rc;
    Lane& L = c->lanes[0];
    GatherGenParams g;
    memset(&g, 0, sizeof g);
    g.gtris = c->derived.g_tris.as<float4>();
    g.rays = L.rays.as<float4>();
    g.oxz = c->g_oxz.as<float2>();
    g.tmax = c->g_tmax.as<float>();
    g.w = c->g_w.as<double>();
    g.fx = prm->from[0]; g.fy = prm->from[1]; g.fz = prm->from[2];
    g.tx = prm->to[0]; g.ty = prm->to[1]; g.tz = prm->to[2];
    g.light_length = prm->light_length;
    g.seed_hash = host_wang_hash(prm->seed);
    g.samples = S;
    g.seed = prm->seed;
    g.mode = c->gather_sampling;
    const int rc = for_tri_chunks(c, S, tri_count, [&](int32_t done, int32_t cnt) -> int {
        g.first_tri = first_tri + done;
        g.tri_count = cnt;
        if (sided) launch_gather_generate_faces(g, c->g_face.as<uint8_t>(), c->stream);
        else launch_gather_generate(g, c->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = trace_shadow_rays(c, (int64_t)cnt * S, "uvrt_gather_direct")) return rc;
        if (var)
            launch_gather_reduce_var(g.gtris, g.w, c->g_occ.as<uint8_t>(), c->derived.expected.as<double>(), c->derived.variance.as<double>(),
                                     g.first_tri, cnt, S, prm->photons_equiv, g.mode, c->stream);
        else
            launch_gather_reduce(g.gtris, g.w, c->g_occ.as<uint8_t>(), c->derived.expected.as<double>(), g.first_tri, cnt, S,
                                 prm->photons_equiv, c->stream);
        if (sided)
            launch_gather_reduce_faces(g.gtris, g.w, c->g_occ.as<uint8_t>(), c->g_face.as<uint8_t>(), c->derived.faces.as<double>(),
                                       g.first_tri, cnt, S, prm->photons_equiv, c->T, c->stream);
        HIP_TRY(hipGetLastError());
        return UVRT_OK;
    });
    if (rc) return rc;
    if (var) {
        uvrt_ctx::GatherMemo m;
        m.valid = true;
        m.first = first_tri; m.count = tri_count; m.samples = S; m.mode = g.mode; m.photons_equiv = prm->photons_equiv;
        m.seed = prm->seed;
        memcpy(m.from, prm->from, 12);
        memcpy(m.to, prm->to, 12);
        m.light_length = prm->light_length;
        c->derived.gather_memo = m;
    }
    return UVRT_OK;
}

int uvrt_accumulate_expected(uvrt_ctx* c, float time_step, int32_t tri_count)
{
    if (!c || !c->have_scene || tri_count < 0 || tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_accumulate_expected: bad tri_count");
    if (int rc = set_device(c)) return rc;       // (an accumulate that uvrt_accumulate has deferred goes first: launch order)
    if (int rc = join_all(c)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    c->derived.gather_memo = {};                         // the estimate is consumed: nothing left to refine
    c->ext_touch_maps = false;                   // (on the context's stream, behind the caller's work: the fence below covers it)
    launch_accumulate_expected(c->photon_map.as<double>(), c->max_map.as<double>(), c->derived.expected.as<double>(), time_step,
                               tri_count, c->stream);
    HIP_TRY(hipGetLastError());
    // the variance of the estimate that has just been consumed goes with it: a stale one is never paired with a later estimate
    if (c->derived.variance.p && tri_count > 0) HIP_TRY(hipMemsetAsync(c->derived.variance.p, 0, (size_t)tri_count * 8, c->stream));
    if (c->derived.faces.p && tri_count > 0)     // ... and so do its face planes
        for (int f = 0; f < 2; ++f)
            HIP_TRY(hipMemsetAsync(c->derived.faces.as<double>() + (size_t)f * (size_t)c->T, 0, (size_t)tri_count * 8, c->stream));
    return mark_map_fence(c);                    // later accumulate / Shade work on a side lane waits for it
}

// uvrt_read_expected / uvrt_write_expected and their variance twins: a range of the expected or the variance plane (made,
// zeroed, by whichever call comes first)
static int plane_range(uvrt_ctx* c, const char* who, bool variance, void* host, int32_t first, int32_t count, hipMemcpyKind kind)
{
    if (!c || !host) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (!range_ok(host, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->T);
    if (int rc = set_device(c)) return rc;
    if (int rc = variance ? ensure_variance(c) : ensure_expected(c)) return rc;
    if (kind == hipMemcpyHostToDevice) c->derived.gather_memo = {};     // the planes are the caller's now, not the remembered gather's
    return range_copy(c, variance ? c->derived.variance.p : c->derived.expected.p, 8, host, first, count, kind);
}

int uvrt_read_expected(uvrt_ctx* c, double* out, int32_t first, int32_t count)
{
    return plane_range(c, "uvrt_read_expected", false, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_write_expected(uvrt_ctx* c, const double* in, int32_t first, int32_t count)
{
    return plane_range(c, "uvrt_write_expected", false, const_cast<double*>(in), first, count, hipMemcpyHostToDevice);
}

int uvrt_read_variance(uvrt_ctx* c, double* out, int32_t first, int32_t count)
{
    return plane_range(c, "uvrt_read_variance", true, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_write_variance(uvrt_ctx* c, const double* in, int32_t first, int32_t count)
{
    return plane_range(c, "uvrt_write_variance", true, const_cast<double*>(in), first, count, hipMemcpyHostToDevice);
}

// a range of face plane `face`; unlike the write calls above, the write leaves the remembered gather: it touches neither plane
// a refine works on
static int faces_range(uvrt_ctx* c, const char* who, int32_t face, void* host, int32_t first, int32_t count, hipMemcpyKind kind)
{
    if (!c || !host) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (face != 0 && face != 1) return fail(UVRT_ERR_INVALID, "%s: face must be 0 or 1, not %d", who, face);
    if (!range_ok(host, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->T);
    if (int rc = set_device(c)) return rc;
    if (int rc = ensure_faces(c)) return rc;
    return range_copy(c, c->derived.faces.as<double>() + (size_t)face * (size_t)c->T, 8, host, first, count, kind);
}

int uvrt_read_gather_faces(uvrt_ctx* c, int32_t face, double* out, int32_t first, int32_t count)
{
    return faces_range(c, "uvrt_read_gather_faces", face, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_write_gather_faces(uvrt_ctx* c, int32_t face, const double* in, int32_t first, int32_t count)
{
    return faces_range(c, "uvrt_write_gather_faces", face, const_cast<double*>(in), first, count, hipMemcpyHostToDevice);
}

int uvrt_gather_refine(uvrt_ctx* c, const uvrt_refine_params* prm, int32_t first_tri, int32_t tri_count, uvrt_refine_report* report)
{
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: no scene");
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: shadow rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", c->flavour);
    const uvrt_ctx::GatherMemo m = c->derived.gather_memo;
    if (!m.valid)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: no remembered gather (uvrt_gather_direct with uvrt_set_gather_variance(1), not yet refined or consumed)");
    if (first_tri < m.first || tri_count < 0 || (int64_t)first_tri + tri_count > (int64_t)m.first + m.count)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: triangles [%d, +%d) outside the remembered gather's [%d, +%d)", first_tri,
                    tri_count, m.first, m.count);
    if (int rc = check_refine_params(c, prm, "uvrt_gather_refine")) return rc;
    const int32_t M = prm->max_extra;
    if ((int64_t)M > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: max_extra = %d exceeds the ray capacity %lld (uvrt_resize_rays)", M, (long long)c->capacity);
    if (prm->seed == m.seed)
        return fail(UVRT_ERR_INVALID, "uvrt_gather_refine: seed %u is the refined gather's: the extra samples would repeat its own", prm->seed);
    if (int rc = set_device(c)) return rc;
    if (int rc = begin_shadow_launch(c)) return rc;
    const size_t cap = (size_t)c->capacity;
    if (int rc = c->g_w.ensure(cap * 8, false, c->stream)) return rc;
    if (int rc = ensure_refine_buffers(c)) return rc;
    if (report) *report = {};
    // (the remembered gather made g_tris and both planes, and whatever releases them -- uvrt_set_scene -- forgets it)
    const float4* gtris = c->derived.g_tris.as<float4>();
    int32_t* offs = c->g_offs.as<int32_t>();
    launch_refine_count(gtris, c->derived.expected.as<double>(), c->derived.variance.as<double>(), c->derived.g_extra.as<int32_t>(), c->T, first_tri,
                        tri_count, m.samples, prm->rel_error, prm->min_expected, M, c->stream);
    launch_refine_scan(c->derived.g_extra.as<int32_t>(), offs, c->g_scan.as<int32_t>(), first_tri, tri_count, c->stream);
    HIP_TRY(hipGetLastError());
    // the call's one round trip: the offsets, to cut the range into chunks of at most `capacity` rays
    std::vector<int32_t> h((size_t)tri_count + 1);
    if (int rc = copy_sync(c, h.data(), offs, h.size() * 4, hipMemcpyDeviceToHost)) return rc;
    c->derived.gather_memo = {};                    // one refine per gather
    Lane& L = c->lanes[0];
    GatherGenParams g;
    memset(&g, 0, sizeof g);
    g.gtris = gtris;
    g.rays = L.rays.as<float4>();
    g.oxz = c->g_oxz.as<float2>();
    g.tmax = c->g_tmax.as<float>();
    g.w = c->g_w.as<double>();
    g.fx = m.from[0]; g.fy = m.from[1]; g.fz = m.from[2];
    g.tx = m.to[0]; g.ty = m.to[1]; g.tz = m.to[2];
    g.light_length = m.light_length;
    g.seed_hash = host_wang_hash(prm->seed);
    g.first_tri = first_tri;
    g.tri_count = tri_count;
    g.seed = prm->seed;
    g.mode = m.mode;
    // chunks, greedily from consecutive triangles: a triangle's samples never straddle two of them (n_t <= max_extra <=
    // capacity, so every chunk takes at least one triangle), and the chunking shows in no bit
    int32_t refined = 0;
    for (int32_t lo = 0; lo < tri_count;) {
        int32_t hi = lo + 1;
        while (hi < tri_count && (int64_t)h[hi + 1] - h[lo] <= c->capacity) ++hi;
        const int32_t rays = h[hi] - h[lo];
        for (int32_t i = lo; i < hi; ++i) refined += h[i + 1] > h[i];
        if (rays > 0) {
            launch_refine_generate(g, offs, lo, hi, rays, c->stream);
            HIP_TRY(hipGetLastError());
            if (int rc = trace_shadow_rays(c, rays, "uvrt_gather_refine")) return rc;
            launch_refine_reduce(gtris, g.w, c->g_occ.as<uint8_t>(), offs, c->derived.expected.as<double>(), c->derived.variance.as<double>(),
                                 first_tri, lo, hi, m.samples, m.photons_equiv, m.mode, c->stream);
            HIP_TRY(hipGetLastError());
        }
        lo = hi;
    }
    if (report) { report->extra_rays = h[tri_count]; report->refined = refined; }
    return UVRT_OK;
}

int uvrt_read_gather_extra(uvrt_ctx* c, int32_t* out, int32_t first, int32_t count)
{
    if (!c || !out) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_extra: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_extra: no scene");
    if (!range_ok(out, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "uvrt_read_gather_extra: range [%d,+%d) outside [0,%d)", first, count, c->T);
    if (int rc = set_device(c)) return rc;
    if (int rc = c->derived.g_extra.ensure((size_t)c->T * 4, true, c->stream)) return rc;
    return range_copy(c, c->derived.g_extra.p, 4, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_refine_counts(uvrt_ctx* c, int32_t samples0, const uvrt_refine_params* prm, int32_t first_tri, int32_t tri_count,
                       int32_t* offsets_out)
{
    if (!c || !prm || !offsets_out) return fail(UVRT_ERR_INVALID, "uvrt_refine_counts: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_refine_counts: no scene");
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "uvrt_refine_counts: shadow rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", c->flavour);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_refine_counts: triangles [%d, +%d) outside [0, %d]", first_tri, tri_count, c->T);
    if (samples0 < 2 || samples0 > 4096)
        return fail(UVRT_ERR_INVALID, "uvrt_refine_counts: samples0 = %d must be in [2, 4096], a gather's with the variance on", samples0);
    if (int rc = check_refine_params(c, prm, "uvrt_refine_counts")) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;        // behind all outstanding work; "the last generate" and the remembered gather stay
    if (int rc = ensure_expected(c)) return rc;
    if (int rc = ensure_variance(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    if (int rc = ensure_refine_buffers(c)) return rc;
    // the two launches of uvrt_gather_refine, on the planes as they are
    launch_refine_count(c->derived.g_tris.as<float4>(), c->derived.expected.as<double>(), c->derived.variance.as<double>(), c->derived.g_extra.as<int32_t>(), c->T,
                        first_tri, tri_count, samples0, prm->rel_error, prm->min_expected, prm->max_extra, c->stream);
    launch_refine_scan(c->derived.g_extra.as<int32_t>(), c->g_offs.as<int32_t>(), c->g_scan.as<int32_t>(), first_tri, tri_count, c->stream);
    HIP_TRY(hipGetLastError());
    return copy_sync(c, offsets_out, c->g_offs.p, ((size_t)tri_count + 1) * 4, hipMemcpyDeviceToHost);
}

}  // extern "C"

// uvrt_capi_indirect.hip -- closest hits and the one-bounce gather (include/uvrt.h "one diffuse bounce"): uvrt_closest_hits,
// uvrt_indirect_source_from_expected, uvrt_read_indirect_source, uvrt_write_indirect_source, uvrt_gather_indirect,
// uvrt_gather_indirect_rays (uvrt_indirect.hip's kernels)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

int ensure_source(uvrt_ctx* c)
{
    return c->derived.source.ensure((size_t)c->T * 8, true, c->stream);
}

// begin_shadow_launch plus the hit records
int begin_closest_launch(uvrt_ctx* c)
{
    if (int rc = begin_shadow_launch(c)) return rc;
    return c->g_hit.ensure((size_t)std::max<int64_t>(c->capacity, 1) * 8, false, c->stream);
}

// k_closest_free over the first n rays of lane 0 (rays, g_oxz, g_tmax -> g_hit) on the context's stream
int trace_closest_rays(uvrt_ctx* c, int64_t n, const char* who)
{
    ClosestParams cp;
    fill_query_launch(c, cp, n);
    cp.hit = c->g_hit.as<uint2>();
    return timed_launch(c, c->stream, who, "the closest-hit launch",
                        [&] { return launch_closest_free(cp, variant_per_cu(c->variant, 8), c->stream); });
}

// the arguments uvrt_gather_indirect and uvrt_gather_indirect_rays share; `who` names the call in the message
int check_indirect(uvrt_ctx* c, const uvrt_indirect_params* prm, int32_t first_tri, int32_t tri_count, const char* who)
{
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "%s: closest hits are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", who, c->flavour);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "%s: triangles [%d, +%d) outside [0, %d]", who, first_tri, tri_count, c->T);
    const int32_t S = prm->samples;
    if (S < 2 || S > 4096 || (S & 1)) return fail(UVRT_ERR_INVALID, "%s: samples = %d must be even and in [2, 4096]", who, S);
    if ((int64_t)S > c->capacity)
        return fail(UVRT_ERR_INVALID, "%s: samples = %d exceed the ray capacity %lld (uvrt_resize_rays)", who, S, (long long)c->capacity);
    if ((int64_t)c->T * S >= ((int64_t)1 << 31))
        return fail(UVRT_ERR_INVALID, "%s: %d triangles x %d samples do not fit 2^31 sample numbers", who, c->T, S);
    if (!std::isfinite(prm->reflectance) || !(prm->reflectance >= 0.0f) || !(prm->reflectance <= 1.0f))
        return fail(UVRT_ERR_INVALID, "%s: reflectance must be finite and in [0, 1]", who);
    if (prm->add != 0 && prm->add != 1) return fail(UVRT_ERR_INVALID, "%s: add must be 0 or 1, not %d", who, prm->add);
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return fail(UVRT_ERR_INVALID, "%s: reserved fields must be 0", who);
    return UVRT_OK;
}

IndirectGenParams indirect_gen_params(uvrt_ctx* c, const uvrt_indirect_params* prm)
{
    IndirectGenParams g;
    memset(&g, 0, sizeof g);
    g.gtris = c->derived.g_tris.as<float4>();
    g.rays = c->lanes[0].rays.as<float4>();
    g.oxz = c->g_oxz.as<float2>();
    g.tmax = c->g_tmax.as<float>();
    g.seed_hash = host_wang_hash(prm->seed);
    g.samples = prm->samples;
    return g;
}

static int source_range(uvrt_ctx* c, const char* who, void* host, int32_t first, int32_t count, hipMemcpyKind kind)
{
    if (!c || !host) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (!range_ok(host, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->T);
    if (int rc = set_device(c)) return rc;
    if (int rc = ensure_source(c)) return rc;
    return range_copy(c, c->derived.source.p, 8, host, first, count, kind);
}

}  // namespace uvrt_impl

extern "C" {

int uvrt_closest_hits(uvrt_ctx* c, const void* rays32, int64_t n, float* dist_out, int32_t* tri_out)
{
    if (!c || !rays32 || !dist_out || !tri_out) return fail(UVRT_ERR_INVALID, "uvrt_closest_hits: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_closest_hits: no scene");
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "uvrt_closest_hits: closest hits are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", c->flavour);
    if (n < 0 || n > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_closest_hits: n = %lld exceeds the ray capacity %lld (uvrt_resize_rays)", (long long)n,
                    (long long)c->capacity);
    if (n == 0) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    if (int rc = upload_query_rays(c, rays32, n, begin_closest_launch)) return rc;
    if (int rc = trace_closest_rays(c, n, "uvrt_closest_hits")) return rc;
    std::vector<uint32_t> h((size_t)n * 2);
    if (int rc = copy_sync(c, h.data(), c->g_hit.p, (size_t)n * 8, hipMemcpyDeviceToHost)) return rc;
    for (int64_t i = 0; i < n; ++i) {
        memcpy(&dist_out[i], &h[2 * i], 4);
        tri_out[i] = (int32_t)h[2 * i + 1];     // 0xFFFFFFFF: -1
    }
    return UVRT_OK;
}

int uvrt_indirect_source_from_expected(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_indirect_source_from_expected: null context");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_indirect_source_from_expected: no scene");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    if (int rc = ensure_source(c)) return rc;
    if (c->T > 0)
        HIP_TRY(hipMemcpyAsync(c->derived.source.p, c->derived.expected.p, (size_t)c->T * 8, hipMemcpyDeviceToDevice, c->stream));
    return UVRT_OK;
}

int uvrt_read_indirect_source(uvrt_ctx* c, double* out, int32_t first, int32_t count)
{
    return source_range(c, "uvrt_read_indirect_source", out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_write_indirect_source(uvrt_ctx* c, const double* in, int32_t first, int32_t count)
{
    return source_range(c, "uvrt_write_indirect_source", const_cast<double*>(in), first, count, hipMemcpyHostToDevice);
}

int uvrt_gather_indirect(uvrt_ctx* c, const uvrt_indirect_params* prm, int32_t first_tri, int32_t tri_count)
{
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "uvrt_gather_indirect: null argument");
    if (int rc = check_indirect(c, prm, first_tri, tri_count, "uvrt_gather_indirect")) return rc;
    if (int rc = set_device(c)) return rc;
    c->derived.gather_memo = {};                    // the expected plane is no longer the remembered gather's
    if (int rc = begin_closest_launch(c)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    if (int rc = ensure_source(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    const int32_t S = prm->samples;
    IndirectGenParams g = indirect_gen_params(c, prm);
    IndirectReduceParams r;
    memset(&r, 0, sizeof r);
    r.gtris = g.gtris;
    r.source = c->derived.source.as<double>();
    r.hit = c->g_hit.as<uint2>();
    r.expected = c->derived.expected.as<double>();
    r.samples = S;
    r.T = c->T;
    r.reflectance = prm->reflectance;
    r.add = prm->add;
    return for_tri_chunks(c, S, tri_count, [&](int32_t done, int32_t cnt) -> int {
        g.first_tri = r.first_tri = first_tri + done;
        g.tri_count = r.tri_count = cnt;
        launch_indirect_generate(g, c->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = trace_closest_rays(c, (int64_t)cnt * S, "uvrt_gather_indirect")) return rc;
        launch_indirect_reduce(r, c->stream);
        HIP_TRY(hipGetLastError());
        return UVRT_OK;
    });
}

int uvrt_gather_indirect_rays(uvrt_ctx* c, const uvrt_indirect_params* prm, int32_t first_tri, int32_t tri_count, void* rays32_out)
{
    if (!c || !prm || !rays32_out) return fail(UVRT_ERR_INVALID, "uvrt_gather_indirect_rays: null argument");
    if (int rc = check_indirect(c, prm, first_tri, tri_count, "uvrt_gather_indirect_rays")) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = begin_closest_launch(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    const int32_t S = prm->samples;
    const int32_t per_chunk = tris_per_chunk(c, S);
    DevBuf out;                                     // one chunk of 32-byte records
    if (int rc = out.ensure((size_t)std::min<int64_t>(per_chunk, std::max(tri_count, 1)) * S * 32, false, c->stream)) return rc;
    IndirectGenParams g = indirect_gen_params(c, prm);
    const int rc = for_tri_chunks(c, S, tri_count, [&](int32_t done, int32_t cnt) -> int {
        const int64_t n = (int64_t)cnt * S;
        g.first_tri = first_tri + done;
        g.tri_count = cnt;
        launch_indirect_generate(g, c->stream);
        launch_export_closest_rays(g.rays, g.oxz, g.tmax, out.p, n, c->stream);
        HIP_TRY(hipGetLastError());
        return copy_sync(c, (char*)rays32_out + (size_t)done * S * 32, out.p, (size_t)n * 32, hipMemcpyDeviceToHost);
    });
    if (rc) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UVRT_OK;
}

}  // extern "C"

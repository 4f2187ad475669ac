// uvrt_capi_mirror.hip -- specular panels and the mirror gather (include/uvrt.h "specular panels"): uvrt_set_mirrors,
// uvrt_mirror_info, uvrt_read_mirrors, uvrt_drop_mirrors, uvrt_gather_mirror (uvrt_mirror.hip's kernels between the closest-hit
// and the shadow-ray launches of uvrt_capi_indirect.hip and uvrt_capi_gather.hip)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

extern "C" {

int uvrt_set_mirrors(uvrt_ctx* c, const uvrt_mirror* panels, int32_t count, const uint8_t* panel_of_tri)
{
    const char* who = "uvrt_set_mirrors";
    if (!c || !panels || !panel_of_tri) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (count < 1 || count > UVRT_MIRROR_MAX)
        return fail(UVRT_ERR_INVALID, "%s: count = %d must be in [1, %d]", who, count, UVRT_MIRROR_MAX);
    MirrorPanel planes[UVRT_MIRROR_MAX] = {};
    for (int32_t k = 0; k < count; ++k) {
        const uvrt_mirror& m = panels[k];
        for (int a = 0; a < 3; ++a)
            if (!std::isfinite(m.point[a]) || !std::isfinite(m.normal[a]))
                return fail(UVRT_ERR_INVALID, "%s: panel %d has a non-finite point or normal", who, k);
        if (!std::isfinite(m.reflectance) || !(m.reflectance >= 0.0f) || !(m.reflectance <= 1.0f))
            return fail(UVRT_ERR_INVALID, "%s: panel %d: reflectance must be finite and in [0, 1]", who, k);
        if (m.reserved != 0) return fail(UVRT_ERR_INVALID, "%s: panel %d: reserved must be 0", who, k);
        const double nx = (double)m.normal[0], ny = (double)m.normal[1], nz = (double)m.normal[2];
        const double len = std::sqrt((nx * nx + ny * ny) + nz * nz);
        if (!(len > 0.0)) return fail(UVRT_ERR_INVALID, "%s: panel %d has a zero normal", who, k);
        MirrorPanel& p = planes[k];
        p.qx = (double)m.point[0]; p.qy = (double)m.point[1]; p.qz = (double)m.point[2];
        p.mx = nx / len; p.my = ny / len; p.mz = nz / len;
        p.rho = (double)m.reflectance;
        p.member = k + 1;
    }
    int32_t members = 0;
    for (int32_t t = 0; t < c->T; ++t) {
        if (panel_of_tri[t] > count)
            return fail(UVRT_ERR_INVALID, "%s: panel_of_tri[%d] = %d names no panel of %d", who, t, (int)panel_of_tri[t], count);
        members += panel_of_tri[t] != 0;
    }
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    auto& d = c->derived;
    if (int rc = d.panel_of_tri_dev.ensure((size_t)std::max(c->T, 1), false, c->stream)) return rc;
    if (int rc = copy_sync(c, d.panel_of_tri_dev.p, panel_of_tri, (size_t)c->T, hipMemcpyHostToDevice)) return rc;
    for (int32_t k = 0; k < UVRT_MIRROR_MAX; ++k) {
        d.mirrors[k] = k < count ? panels[k] : uvrt_mirror{};
        d.mirror_planes[k] = planes[k];
    }
    d.mirror_count = count;
    d.mirror_members = members;
    return UVRT_OK;
}

int uvrt_mirror_info(uvrt_ctx* c, int32_t out4[4])
{
    if (!c || !out4) return fail(UVRT_ERR_INVALID, "uvrt_mirror_info: null argument");
    const bool have = c->have_scene && c->derived.mirror_count > 0;
    out4[0] = have ? c->derived.mirror_count : 0;
    out4[1] = have ? c->derived.mirror_members : 0;
    out4[2] = 0;
    out4[3] = 0;
    return UVRT_OK;
}

int uvrt_read_mirrors(uvrt_ctx* c, uvrt_mirror* panels_out, uint8_t* panel_of_tri_out)
{
    const char* who = "uvrt_read_mirrors";
    if (!c || !panels_out || !panel_of_tri_out) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    const auto& d = c->derived;
    if (d.mirror_count <= 0) return fail(UVRT_ERR_INVALID, "%s: no panels (uvrt_set_mirrors)", who);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    memcpy(panels_out, d.mirrors, (size_t)d.mirror_count * sizeof(uvrt_mirror));
    return copy_sync(c, panel_of_tri_out, d.panel_of_tri_dev.p, (size_t)c->T, hipMemcpyDeviceToHost);     // what the kernels read
}

int uvrt_drop_mirrors(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_drop_mirrors: null context");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_drop_mirrors: no scene");
    auto& d = c->derived;
    if (d.mirror_count <= 0) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    d.panel_of_tri_dev.release();                   // (freeing waits for the device)
    d.mirror_count = 0;
    d.mirror_members = 0;
    return UVRT_OK;
}

int uvrt_gather_mirror(uvrt_ctx* c, const uvrt_gather_params* prm, int32_t add, int32_t first_tri, int32_t tri_count)
{
    const char* who = "uvrt_gather_mirror";
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (c->derived.mirror_count <= 0) return fail(UVRT_ERR_INVALID, "%s: no panels (uvrt_set_mirrors)", who);
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "%s: shadow rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", who, c->flavour);
    if (add != 0 && add != 1) return fail(UVRT_ERR_INVALID, "%s: add must be 0 or 1, not %d", who, add);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "%s: triangles [%d, +%d) outside [0, %d]", who, first_tri, tri_count, c->T);
    const int32_t S = prm->samples;
    if (S < 1 || S > 4096) return fail(UVRT_ERR_INVALID, "%s: samples = %d must be in [1, 4096]", who, S);
    if ((int64_t)S > c->capacity)
        return fail(UVRT_ERR_INVALID, "%s: samples = %d exceed the ray capacity %lld (uvrt_resize_rays)", who, S, (long long)c->capacity);
    if ((int64_t)c->T * S >= ((int64_t)1 << 31))
        return fail(UVRT_ERR_INVALID, "%s: %d triangles x %d samples do not fit 2^31 sample numbers", who, c->T, S);
    if (prm->photons_equiv <= 0) return fail(UVRT_ERR_INVALID, "%s: photons_equiv must be > 0", who);
    if (int rc = set_device(c)) return rc;
    c->derived.gather_memo = {};                    // the expected plane is no longer the remembered gather's alone
    if (int rc = begin_closest_launch(c)) return rc;
    const size_t cap = (size_t)c->capacity;
    const bool sided = c->gather_faces != 0;
    if (int rc = c->g_w.ensure(cap * 8, false, c->stream)) return rc;
    if (int rc = c->g_face.ensure(cap, false, c->stream)) return rc;
    if (int rc = c->g_point.ensure(cap * 16, false, c->stream)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    if (sided)
        if (int rc = ensure_faces(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    MirrorGenParams g;
    memset(&g, 0, sizeof g);
    g.g.gtris = c->derived.g_tris.as<float4>();
    g.g.rays = c->lanes[0].rays.as<float4>();
    g.g.oxz = c->g_oxz.as<float2>();
    g.g.tmax = c->g_tmax.as<float>();
    g.g.w = c->g_w.as<double>();
    g.g.fx = prm->from[0]; g.g.fy = prm->from[1]; g.g.fz = prm->from[2];
    g.g.tx = prm->to[0]; g.g.ty = prm->to[1]; g.g.tz = prm->to[2];
    g.g.light_length = prm->light_length;
    g.g.seed_hash = host_wang_hash(prm->seed);
    g.g.samples = S;
    g.g.seed = prm->seed;
    g.g.mode = c->gather_sampling;
    g.face = c->g_face.as<uint8_t>();
    g.point = c->g_point.as<float4>();
    MirrorFoldParams f;
    memset(&f, 0, sizeof f);
    f.rays = g.g.rays; f.oxz = g.g.oxz; f.tmax = g.g.tmax; f.w = g.g.w;
    f.hit = c->g_hit.as<uint2>();
    f.point = g.point;
    f.panel_of_tri = c->derived.panel_of_tri_dev.as<uint8_t>();
    f.T = c->T;
    MirrorReduceParams r;
    memset(&r, 0, sizeof r);
    r.gtris = g.g.gtris;
    r.w = g.g.w;
    r.occluded = c->g_occ.as<uint8_t>();
    r.face = g.face;
    r.expected = c->derived.expected.as<double>();
    r.faces = sided ? c->derived.faces.as<double>() : nullptr;
    r.samples = S;
    r.photons_equiv = prm->photons_equiv;
    r.T = c->T;
    for (int32_t k = 0; k < c->derived.mirror_count; ++k) {
        g.m = c->derived.mirror_planes[k];
        f.member = k + 1;
        r.accumulate = (add || k > 0) ? 1 : 0;
        const int rc = for_tri_chunks(c, S, tri_count, [&](int32_t done, int32_t cnt) -> int {
            const int64_t n = (int64_t)cnt * S;
            g.g.first_tri = r.first_tri = first_tri + done;
            g.g.tri_count = r.tri_count = cnt;
            f.n = n;
            launch_mirror_generate(g, c->stream);
            HIP_TRY(hipGetLastError());
            if (int rc = trace_closest_rays(c, n, who)) return rc;
            launch_mirror_fold(f, c->stream);
            HIP_TRY(hipGetLastError());
            if (int rc = trace_shadow_rays(c, n, who)) return rc;
            launch_mirror_reduce(r, c->stream);
            HIP_TRY(hipGetLastError());
            return UVRT_OK;
        });
        if (rc) return rc;
    }
    return UVRT_OK;
}

}  // extern "C"

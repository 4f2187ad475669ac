// uvrt_capi_links.hip -- recorded hit links and the multi-bounce gather over them (include/uvrt.h "recorded hit links"):
// uvrt_indirect_links_build, uvrt_indirect_links_info, uvrt_read_indirect_links, uvrt_gather_indirect_linked, and their sided
// forms (include/uvrt.h "face-resolved gather and bounces"): uvrt_indirect_links_build_sided, uvrt_gather_indirect_linked_sided
// (uvrt_links.hip's kernels; the build traces with uvrt_indirect.hip's, through uvrt_capi_indirect.hip's helpers)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

// uvrt_indirect_links_build (kind 0) and uvrt_indirect_links_build_sided (kind 1): one build, two store kernels
static int links_build(uvrt_ctx* c, const uvrt_links_params* prm, int32_t kind, const char* who)
{
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0) return fail(UVRT_ERR_INVALID, "%s: reserved fields must be 0", who);
    uvrt_indirect_params ip;                        // the traced bounce these links stand for
    memset(&ip, 0, sizeof ip);
    ip.samples = prm->samples;
    ip.seed = prm->seed;
    if (int rc = check_indirect(c, &ip, 0, c->T, who)) return rc;
    if (int rc = set_device(c)) return rc;
    if (int rc = begin_closest_launch(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    const int32_t S = prm->samples;
    DevBuf fresh;                                   // the earlier links stay until these are complete
    if (int rc = fresh.ensure((size_t)c->T * (size_t)S * 4, false, c->stream)) return rc;
    IndirectGenParams g = indirect_gen_params(c, &ip);
    LinksStoreParams st;
    memset(&st, 0, sizeof st);
    st.gtris = g.gtris;
    st.hit = c->g_hit.as<uint2>();
    st.links = fresh.as<int32_t>();
    st.samples = S;
    st.T = c->T;
    // uvrt_gather_indirect's chunks: generate -> the closest-hit kernel, then the store
    const int rc = for_tri_chunks(c, S, c->T, [&](int32_t done, int32_t cnt) -> int {
        g.first_tri = st.first_tri = done;
        g.tri_count = st.tri_count = cnt;
        launch_indirect_generate(g, c->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = trace_closest_rays(c, (int64_t)cnt * S, who)) return rc;
        if (kind) launch_links_store_sided(st, g.rays, c->stream);
        else launch_links_store(st, c->stream);
        HIP_TRY(hipGetLastError());
        return UVRT_OK;
    });
    if (rc) return rc;
    c->derived.links = std::move(fresh);            // (freeing the earlier ones waits for the device)
    c->derived.links_samples = S;
    c->derived.links_seed = prm->seed;
    c->derived.links_flavour = c->flavour;
    c->derived.links_kind = kind;
    return UVRT_OK;
}

// uvrt_gather_indirect_linked (kind 0: `source` and plain links) and uvrt_gather_indirect_linked_sided (kind 1: the face planes
// and sided links, every irradiance plane interleaved e[2 * h + face]): the same checks, the same sequence of launches
static int linked_gather(uvrt_ctx* c, const uvrt_linked_params* prm, int32_t first_tri, int32_t tri_count, int32_t kind, const char* who)
{
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    const int32_t S = c->derived.links_samples;
    if (S <= 0)
        return fail(UVRT_ERR_INVALID, "%s: no links (%s)", who, kind ? "uvrt_indirect_links_build_sided" : "uvrt_indirect_links_build");
    if (c->derived.links_kind != kind)
        return fail(UVRT_ERR_INVALID, kind ? "%s: the links are plain: this call reads sided ones (uvrt_indirect_links_build_sided)"
                                           : "%s: the links are sided: this call reads plain ones (uvrt_indirect_links_build)", who);
    const int32_t K = prm->bounces;
    if (K < 1 || K > 16) return fail(UVRT_ERR_INVALID, "%s: bounces = %d must be in [1, 16]", who, K);
    if (!std::isfinite(prm->reflectance) || !(prm->reflectance >= 0.0f) || !(prm->reflectance <= 1.0f))
        return fail(UVRT_ERR_INVALID, "%s: reflectance must be finite and in [0, 1]", who);
    if (prm->add != 0 && prm->add != 1) return fail(UVRT_ERR_INVALID, "%s: add must be 0 or 1, not %d", who, prm->add);
    if (prm->reserved[0] != 0 || prm->reserved[1] != 0 || prm->reserved[2] != 0)
        return fail(UVRT_ERR_INVALID, "%s: reserved fields must be 0", who);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "%s: triangles [%d, +%d) outside [0, %d]", who, first_tri, tri_count, c->T);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    uvrt_ctx::SceneDerived& d = c->derived;
    if (int rc = ensure_expected(c)) return rc;
    if (int rc = kind ? ensure_faces(c) : ensure_source(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    const size_t plane = (size_t)c->T * 8;
    const size_t eplane = kind ? plane * 2 : plane;         // (ensure only ever grows a buffer: the two kinds share link_e)
    if (int rc = d.link_e[0].ensure(eplane, false, c->stream)) return rc;
    if (K > 1) {
        if (int rc = d.link_e[1].ensure(eplane, false, c->stream)) return rc;
        if (int rc = d.link_total.ensure(plane, false, c->stream)) return rc;
    }
    d.gather_memo = {};                             // the expected plane is no longer the remembered gather's
    LinksApplyParams a;
    memset(&a, 0, sizeof a);
    a.gtris = d.g_tris.as<float4>();
    a.links = d.links.as<int32_t>();
    a.samples = S;
    a.T = c->T;
    a.reflectance = prm->reflectance;
    a.add = prm->add;
    if (kind) launch_links_irradiance_sided(a.gtris, d.faces.as<double>(), d.link_e[0].as<double>(), c->T, c->stream);
    else launch_links_irradiance(a.gtris, d.source.as<double>(), d.link_e[0].as<double>(), c->T, c->stream);
    HIP_TRY(hipGetLastError());
    // one launch per bounce; the bounces before the last run over all T triangles: they are the next bounce's source
    for (int32_t b = 1; b <= K; ++b) {
        const bool last = b == K;
        a.e_in = d.link_e[(b - 1) & 1].as<double>();
        a.e_out = last ? nullptr : d.link_e[b & 1].as<double>();
        a.total_in = b == 1 ? nullptr : d.link_total.as<double>();
        a.total_out = last ? nullptr : d.link_total.as<double>();
        a.expected = last ? d.expected.as<double>() : nullptr;
        a.first_tri = last ? first_tri : 0;
        a.tri_count = last ? tri_count : c->T;
        if (kind) launch_links_apply_sided(a, c->stream);
        else launch_links_apply(a, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return UVRT_OK;
}

extern "C" {

int uvrt_indirect_links_build(uvrt_ctx* c, const uvrt_links_params* prm)
{
    return links_build(c, prm, 0, "uvrt_indirect_links_build");
}

int uvrt_indirect_links_build_sided(uvrt_ctx* c, const uvrt_links_params* prm)
{
    return links_build(c, prm, 1, "uvrt_indirect_links_build_sided");
}

int uvrt_indirect_links_info(uvrt_ctx* c, int32_t out4[4])
{
    if (!c || !out4) return fail(UVRT_ERR_INVALID, "uvrt_indirect_links_info: null argument");
    const bool have = c->have_scene && c->derived.links_samples > 0;
    out4[0] = have ? c->derived.links_samples : 0;
    out4[1] = have ? (int32_t)c->derived.links_seed : 0;
    out4[2] = have ? c->derived.links_flavour : 0;
    out4[3] = have ? c->derived.links_kind : 0;
    return UVRT_OK;
}

int uvrt_read_indirect_links(uvrt_ctx* c, int32_t* out, int32_t first_tri, int32_t tri_count)
{
    const char* who = "uvrt_read_indirect_links";
    if (!c || !out) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    const int32_t S = c->derived.links_samples;
    if (S <= 0) return fail(UVRT_ERR_INVALID, "%s: no links (uvrt_indirect_links_build)", who);
    if (!range_ok(out, first_tri, tri_count, c->T))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first_tri, tri_count, c->T);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    if (tri_count == 0) return UVRT_OK;
    DevBuf tmp;                                     // the range, triangle-major
    const size_t bytes = (size_t)tri_count * (size_t)S * 4;
    if (int rc = tmp.ensure(bytes, false, c->stream)) return rc;
    launch_links_export(c->derived.links.as<int32_t>(), tmp.as<int32_t>(), first_tri, tri_count, S, c->T, c->stream);
    HIP_TRY(hipGetLastError());
    return copy_sync(c, out, tmp.p, bytes, hipMemcpyDeviceToHost);
}

int uvrt_gather_indirect_linked(uvrt_ctx* c, const uvrt_linked_params* prm, int32_t first_tri, int32_t tri_count)
{
    return linked_gather(c, prm, first_tri, tri_count, 0, "uvrt_gather_indirect_linked");
}

int uvrt_gather_indirect_linked_sided(uvrt_ctx* c, const uvrt_linked_params* prm, int32_t first_tri, int32_t tri_count)
{
    return linked_gather(c, prm, first_tri, tri_count, 1, "uvrt_gather_indirect_linked_sided");
}

}  // extern "C"

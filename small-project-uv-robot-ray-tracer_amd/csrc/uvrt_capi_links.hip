// uvrt_capi_links.hip -- recorded hit links and the multi-bounce gather over them (include/uvrt.h "recorded hit links"):
// uvrt_indirect_links_build, uvrt_indirect_links_info, uvrt_read_indirect_links, uvrt_gather_indirect_linked, and their sided
// forms (include/uvrt.h "face-resolved gather and bounces"): uvrt_indirect_links_build_sided, uvrt_gather_indirect_linked_sided
// (uvrt_links.hip's kernels; the build traces with uvrt_indirect.hip's, through uvrt_capi_indirect.hip's helpers); the
// reflectance planes and the gather that reads them (include/uvrt.h "per-face reflectance"): uvrt_fill_reflectance,
// uvrt_write_reflectance, uvrt_read_reflectance, uvrt_reflectance_info, uvrt_drop_reflectance, uvrt_gather_indirect_linked_mapped
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

// What the three linked gathers (uvrt_gather_indirect_linked, its sided form and uvrt_gather_indirect_linked_mapped) share.
// linked_check: the refusals, in the order the calls have always made them; `kind` is the link set the call reads, `reflectance`
// the one rho of the calls that take one (null: the mapped call, which needs the reflectance planes instead).
static int linked_check(uvrt_ctx* c, const void* prm, int32_t kind, int32_t K, const float* reflectance, int32_t add, bool reserved_zero,
                        int32_t first_tri, int32_t tri_count, const char* who)
{
    if (!c || !prm) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (c->derived.links_samples <= 0)
        return fail(UVRT_ERR_INVALID, "%s: no links (%s)", who, kind ? "uvrt_indirect_links_build_sided" : "uvrt_indirect_links_build");
    if (c->derived.links_kind != kind)
        return fail(UVRT_ERR_INVALID, kind ? "%s: the links are plain: this call reads sided ones (uvrt_indirect_links_build_sided)"
                                           : "%s: the links are sided: this call reads plain ones (uvrt_indirect_links_build)", who);
    if (!reflectance && !c->derived.have_rho)
        return fail(UVRT_ERR_INVALID, "%s: no reflectance planes (uvrt_fill_reflectance, uvrt_write_reflectance)", who);
    if (K < 1 || K > 16) return fail(UVRT_ERR_INVALID, "%s: bounces = %d must be in [1, 16]", who, K);
    if (reflectance && (!std::isfinite(*reflectance) || !(*reflectance >= 0.0f) || !(*reflectance <= 1.0f)))
        return fail(UVRT_ERR_INVALID, "%s: reflectance must be finite and in [0, 1]", who);
    if (add != 0 && add != 1) return fail(UVRT_ERR_INVALID, "%s: add must be 0 or 1, not %d", who, add);
    if (!reserved_zero) return fail(UVRT_ERR_INVALID, "%s: reserved fields must be 0", who);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "%s: triangles [%d, +%d) outside [0, %d]", who, first_tri, tri_count, c->T);
    return UVRT_OK;
}

// linked_begin: behind all outstanding launches, the planes the call reads and writes and the ping-pong planes of K bounces
// (kind 1: interleaved e[2 * h + face], twice the size; ensure only ever grows a buffer, so the kinds share link_e)
static int linked_begin(uvrt_ctx* c, int32_t kind, int32_t K)
{
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    uvrt_ctx::SceneDerived& d = c->derived;
    if (int rc = ensure_expected(c)) return rc;
    if (int rc = kind ? ensure_faces(c) : ensure_source(c)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    const size_t plane = (size_t)c->T * 8;
    const size_t eplane = kind ? plane * 2 : plane;
    if (int rc = d.link_e[0].ensure(eplane, false, c->stream)) return rc;
    if (K > 1) {
        if (int rc = d.link_e[1].ensure(eplane, false, c->stream)) return rc;
        if (int rc = d.link_total.ensure(plane, false, c->stream)) return rc;
    }
    d.gather_memo = {};                             // the expected plane is no longer the remembered gather's
    return UVRT_OK;
}

// linked_bounces: one launch per bounce over link_e[0] -> link_e[1] -> link_e[0] ..; the bounces before the last run over all T
// triangles: they are the next bounce's source.  `in` / `out`: the members of the apply kernel's params that take the planes.
template <class Params, class Launch>
static int linked_bounces(uvrt_ctx* c, Params& a, const double* Params::*in, double* Params::*out, int32_t K, int32_t first_tri,
                          int32_t tri_count, Launch&& launch)
{
    uvrt_ctx::SceneDerived& d = c->derived;
    for (int32_t b = 1; b <= K; ++b) {
        const bool last = b == K;
        a.*in = d.link_e[(b - 1) & 1].as<double>();
        a.*out = last ? nullptr : d.link_e[b & 1].as<double>();
        a.total_in = b == 1 ? nullptr : d.link_total.as<double>();
        a.total_out = last ? nullptr : d.link_total.as<double>();
        a.expected = last ? d.expected.as<double>() : nullptr;
        a.first_tri = last ? first_tri : 0;
        a.tri_count = last ? tri_count : c->T;
        launch(a, c->stream);
        HIP_TRY(hipGetLastError());
    }
    return UVRT_OK;
}

// uvrt_gather_indirect_linked (kind 0: `source` and plain links) and uvrt_gather_indirect_linked_sided (kind 1: the face planes
// and sided links, every irradiance plane interleaved e[2 * h + face]): the same checks, the same sequence of launches
static int linked_gather(uvrt_ctx* c, const uvrt_linked_params* prm, int32_t first_tri, int32_t tri_count, int32_t kind, const char* who)
{
    if (int rc = linked_check(c, prm, kind, prm ? prm->bounces : 0, prm ? &prm->reflectance : nullptr, prm ? prm->add : 0,
                              prm && prm->reserved[0] == 0 && prm->reserved[1] == 0 && prm->reserved[2] == 0, first_tri, tri_count, who))
        return rc;
    if (int rc = linked_begin(c, kind, prm->bounces)) return rc;
    uvrt_ctx::SceneDerived& d = c->derived;
    LinksApplyParams a;
    memset(&a, 0, sizeof a);
    a.gtris = d.g_tris.as<float4>();
    a.links = d.links.as<int32_t>();
    a.samples = d.links_samples;
    a.T = c->T;
    a.reflectance = prm->reflectance;
    a.add = prm->add;
    if (kind) launch_links_irradiance_sided(a.gtris, d.faces.as<double>(), d.link_e[0].as<double>(), c->T, c->stream);
    else launch_links_irradiance(a.gtris, d.source.as<double>(), d.link_e[0].as<double>(), c->T, c->stream);
    HIP_TRY(hipGetLastError());
    return linked_bounces(c, a, &LinksApplyParams::e_in, &LinksApplyParams::e_out, prm->bounces, first_tri, tri_count,
                          kind ? launch_links_apply_sided : launch_links_apply);
}

// uvrt_gather_indirect_linked_mapped: the sided sequence with the reflectance planes in place of one rho; the ping-pong planes
// hold radiosities (rho x irradiance) instead of irradiances
static int mapped_gather(uvrt_ctx* c, const uvrt_mapped_params* prm, int32_t first_tri, int32_t tri_count)
{
    const char* who = "uvrt_gather_indirect_linked_mapped";
    if (int rc = linked_check(c, prm, 1, prm ? prm->bounces : 0, nullptr, prm ? prm->add : 0,
                              prm && prm->reserved[0] == 0 && prm->reserved[1] == 0, first_tri, tri_count, who))
        return rc;
    if (int rc = linked_begin(c, 1, prm->bounces)) return rc;
    uvrt_ctx::SceneDerived& d = c->derived;
    LinksMappedParams a;
    memset(&a, 0, sizeof a);
    a.gtris = d.g_tris.as<float4>();
    a.links = d.links.as<int32_t>();
    a.rho = d.rho.as<float>();
    a.samples = d.links_samples;
    a.T = c->T;
    a.add = prm->add;
    launch_links_radiosity_sided(a.gtris, d.faces.as<double>(), a.rho, d.link_e[0].as<double>(), c->T, c->stream);
    HIP_TRY(hipGetLastError());
    return linked_bounces(c, a, &LinksMappedParams::r_in, &LinksMappedParams::r_out, prm->bounces, first_tri, tri_count,
                          launch_links_apply_mapped);
}

// every value finite and in [0, 1] (-0.0f passes as 0)
static bool rho_values_ok(const float* v, int64_t n)
{
    for (int64_t i = 0; i < n; ++i)
        if (!std::isfinite(v[i]) || !(v[i] >= 0.0f) || !(v[i] <= 1.0f)) return false;
    return true;
}

// the planes, made zeroed when absent: an unlisted face absorbs everything
static int ensure_rho(uvrt_ctx* c)
{
    if (c->derived.have_rho) return UVRT_OK;
    c->derived.rho.release();
    if (int rc = c->derived.rho.ensure((size_t)c->T * 8, true, c->stream)) return rc;
    c->derived.have_rho = true;
    return UVRT_OK;
}

extern "C" {

int uvrt_fill_reflectance(uvrt_ctx* c, float rho)
{
    const char* who = "uvrt_fill_reflectance";
    if (!c) return fail(UVRT_ERR_INVALID, "%s: null context", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (!rho_values_ok(&rho, 1)) return fail(UVRT_ERR_INVALID, "%s: reflectance must be finite and in [0, 1]", who);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    if (int rc = ensure_rho(c)) return rc;
    int32_t bits;
    memcpy(&bits, &rho, 4);
    HIP_TRY(hipMemsetD32Async((hipDeviceptr_t)c->derived.rho.p, bits, (size_t)c->T * 2, c->stream));
    return UVRT_OK;
}

int uvrt_write_reflectance(uvrt_ctx* c, int32_t face, const float* in, int32_t first, int32_t count)
{
    const char* who = "uvrt_write_reflectance";
    if (!c || !in) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (face != 0 && face != 1) return fail(UVRT_ERR_INVALID, "%s: face must be 0 or 1, not %d", who, face);
    if (!range_ok(in, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->T);
    if (!rho_values_ok(in, count)) return fail(UVRT_ERR_INVALID, "%s: every reflectance must be finite and in [0, 1]", who);
    if (int rc = set_device(c)) return rc;
    if (int rc = ensure_rho(c)) return rc;
    return range_copy(c, c->derived.rho.as<float>() + (size_t)face * (size_t)c->T, 4, const_cast<float*>(in), first, count,
                      hipMemcpyHostToDevice);
}

int uvrt_read_reflectance(uvrt_ctx* c, int32_t face, float* out, int32_t first, int32_t count)
{
    const char* who = "uvrt_read_reflectance";
    if (!c || !out) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (!c->derived.have_rho) return fail(UVRT_ERR_INVALID, "%s: no reflectance planes (no map is not rho = 0)", who);
    if (face != 0 && face != 1) return fail(UVRT_ERR_INVALID, "%s: face must be 0 or 1, not %d", who, face);
    if (!range_ok(out, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "%s: range [%d,+%d) outside [0,%d)", who, first, count, c->T);
    return range_copy(c, c->derived.rho.as<float>() + (size_t)face * (size_t)c->T, 4, out, first, count, hipMemcpyDeviceToHost);
}

int uvrt_reflectance_info(uvrt_ctx* c, int32_t* have)
{
    if (!c || !have) return fail(UVRT_ERR_INVALID, "uvrt_reflectance_info: null argument");
    *have = c->have_scene && c->derived.have_rho ? 1 : 0;
    return UVRT_OK;
}

int uvrt_drop_reflectance(uvrt_ctx* c)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_drop_reflectance: null context");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_drop_reflectance: no scene");
    if (!c->derived.have_rho) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    c->derived.rho.release();                       // (freeing waits for the device)
    c->derived.have_rho = false;
    return UVRT_OK;
}

int uvrt_gather_indirect_linked_mapped(uvrt_ctx* c, const uvrt_mapped_params* prm, int32_t first_tri, int32_t tri_count)
{
    return mapped_gather(c, prm, first_tri, tri_count);
}

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

// uvrt_capi_gather_batch.hip -- the batched direct gather (include/uvrt.h "batched direct gather"):
// uvrt_gather_direct_batch, uvrt_gather_batch_select, uvrt_gather_batch_info, uvrt_read_gather_batch (uvrt_gather_batch.hip's
// kernels around uvrt_occlude.hip's k_occlude_free)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

using GatherBatch = uvrt_ctx::SceneDerived::GatherBatch;

extern "C" {

int uvrt_gather_direct_batch(uvrt_ctx* c, const uvrt_gather_params* launches, int32_t count, int32_t first_tri, int32_t tri_count)
{
    const char* who = "uvrt_gather_direct_batch";
    if (!c || !launches) return fail(UVRT_ERR_INVALID, "%s: null argument", who);
    if (count < 1 || count > UVRT_GATHER_BATCH_MAX)
        return fail(UVRT_ERR_INVALID, "%s: count = %d must be in [1, %d]", who, count, UVRT_GATHER_BATCH_MAX);
    if (c->gather_faces != 0)
        return fail(UVRT_ERR_INVALID, "%s: a batch keeps no face planes: switch uvrt_set_gather_faces off, or gather launch by launch", who);
    // every launch as uvrt_gather_direct checks it
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "%s: no scene", who);
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "%s: shadow rays are traced in flavours 0 and 1 only (uvrt_set_flavour %d)", who, c->flavour);
    if (first_tri < 0 || tri_count < 0 || (int64_t)first_tri + tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "%s: triangles [%d, +%d) outside [0, %d]", who, first_tri, tri_count, c->T);
    const int32_t S = launches[0].samples;
    const bool var = c->gather_variance != 0;
    for (int32_t k = 0; k < count; ++k) {
        const int32_t Sk = launches[k].samples;
        if (Sk < 1 || Sk > 4096) return fail(UVRT_ERR_INVALID, "%s: launch %d: samples = %d must be in [1, 4096]", who, k, Sk);
        if (var && Sk < 2)
            return fail(UVRT_ERR_INVALID, "%s: launch %d: the variance plane needs samples >= 2 (uvrt_set_gather_variance), not %d", who,
                        k, Sk);
        if ((int64_t)Sk > c->capacity)
            return fail(UVRT_ERR_INVALID, "%s: launch %d: samples = %d exceed the ray capacity %lld (uvrt_resize_rays)", who, k, Sk,
                        (long long)c->capacity);
        if ((int64_t)c->T * Sk >= ((int64_t)1 << 31))
            return fail(UVRT_ERR_INVALID, "%s: launch %d: %d triangles x %d samples do not fit 2^31 sample numbers", who, k, c->T, Sk);
        if (launches[k].photons_equiv <= 0) return fail(UVRT_ERR_INVALID, "%s: launch %d: photons_equiv must be > 0", who, k);
        if (Sk != S) return fail(UVRT_ERR_INVALID, "%s: launch %d: samples = %d, launch 0 has %d: a batch has one sample count", who, k, Sk, S);
    }
    if (int rc = set_device(c)) return rc;
    GatherBatch& B = c->derived.gather_batch;
    B.count = 0;                                    // the earlier batch is dropped; this one counts once its work is enqueued
    if (int rc = begin_shadow_launch(c)) return rc;
    const size_t cap = (size_t)c->capacity;
    if (int rc = c->g_w.ensure(cap * 8, false, c->stream)) return rc;
    if (int rc = ensure_gather_tris(c)) return rc;
    // the planes: zero outside the range (a range that is the whole scene is written entirely)
    const size_t plane_bytes = (size_t)count * (size_t)c->T * 8;
    if (int rc = B.e.ensure(plane_bytes, false, c->stream)) return rc;
    if (var)
        if (int rc = B.v.ensure(plane_bytes, false, c->stream)) return rc;
    if (tri_count < c->T) {
        HIP_TRY(hipMemsetAsync(B.e.p, 0, plane_bytes, c->stream));
        if (var) HIP_TRY(hipMemsetAsync(B.v.p, 0, plane_bytes, c->stream));
    }
    // the launch table, from the context's host buffer (pageable: the copy has read it when the call returns)
    c->gb_host.resize((size_t)count);
    for (int32_t k = 0; k < count; ++k) {
        const uvrt_gather_params& q = launches[k];
        GatherBatchLaunch& r = c->gb_host[(size_t)k];
        memset(&r, 0, sizeof r);
        r.fx = q.from[0]; r.fy = q.from[1]; r.fz = q.from[2];
        r.tx = q.to[0]; r.ty = q.to[1]; r.tz = q.to[2];
        r.light_length = q.light_length;
        r.seed = q.seed;
        r.seed_hash = host_wang_hash(q.seed);
        r.photons_equiv = q.photons_equiv;
    }
    if (int rc = c->gb_table.ensure((size_t)UVRT_GATHER_BATCH_MAX * sizeof(GatherBatchLaunch), false, c->stream)) return rc;
    HIP_TRY(hipMemcpyAsync(c->gb_table.p, c->gb_host.data(), (size_t)count * sizeof(GatherBatchLaunch), hipMemcpyHostToDevice, c->stream));
    GatherBatchParams g;
    memset(&g, 0, sizeof g);
    g.gtris = c->derived.g_tris.as<float4>();
    g.table = c->gb_table.as<GatherBatchLaunch>();
    g.rays = c->lanes[0].rays.as<float4>();
    g.oxz = c->g_oxz.as<float2>();
    g.tmax = c->g_tmax.as<float>();
    g.w = c->g_w.as<double>();
    g.occluded = c->g_occ.as<uint8_t>();
    g.e_planes = B.e.as<double>();
    g.v_planes = var ? B.v.as<double>() : nullptr;
    g.first_tri = first_tri;
    g.tri_count = tri_count;
    g.samples = S;
    g.T = c->T;
    g.mode = c->gather_sampling;
    // pairs q = k * tri_count + lt in chunks of floor(capacity / S), for_tri_chunks' size: a pair's S samples never straddle two
    // of them, so the chunking shows in no bit
    const int64_t pairs = (int64_t)count * tri_count, per_chunk = tris_per_chunk(c, S);
    for (int64_t done = 0; done < pairs; done += per_chunk) {
        g.k0 = (int32_t)(done / tri_count);
        g.lt0 = (int32_t)(done % tri_count);
        g.pair_count = (int32_t)std::min<int64_t>(per_chunk, pairs - done);
        launch_gather_generate_batch(g, c->stream);
        HIP_TRY(hipGetLastError());
        if (int rc = trace_shadow_rays(c, (int64_t)g.pair_count * S, who)) return rc;
        launch_gather_reduce_batch(g, var, c->stream);
        HIP_TRY(hipGetLastError());
    }
    B.count = count;
    B.samples = S;
    B.first = first_tri;
    B.tri_count = tri_count;
    B.mode = g.mode;
    B.flavour = c->flavour;
    B.var = var;
    B.launches.assign(launches, launches + count);
    if (!var) B.v.release();                        // (an earlier batch's)
    return UVRT_OK;
}

int uvrt_gather_batch_select(uvrt_ctx* c, int32_t k)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_gather_batch_select: null context");
    const GatherBatch& B = c->derived.gather_batch;
    if (!c->have_scene || B.count == 0) return fail(UVRT_ERR_INVALID, "uvrt_gather_batch_select: no batch (uvrt_gather_direct_batch)");
    if (k < 0 || k >= B.count) return fail(UVRT_ERR_INVALID, "uvrt_gather_batch_select: k = %d outside the batch's [0, %d)", k, B.count);
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    if (int rc = ensure_expected(c)) return rc;
    if (B.var)
        if (int rc = ensure_variance(c)) return rc;
    c->derived.gather_memo = {};
    const size_t at = ((size_t)k * (size_t)c->T + (size_t)B.first) * 8, bytes = (size_t)B.tri_count * 8;
    if (bytes) {
        HIP_TRY(hipMemcpyAsync((char*)c->derived.expected.p + (size_t)B.first * 8, (const char*)B.e.p + at, bytes, hipMemcpyDeviceToDevice,
                               c->stream));
        if (B.var)
            HIP_TRY(hipMemcpyAsync((char*)c->derived.variance.p + (size_t)B.first * 8, (const char*)B.v.p + at, bytes,
                                   hipMemcpyDeviceToDevice, c->stream));
    }
    if (B.var) {                                    // what uvrt_gather_direct(&launches[k], ..) would remember
        const uvrt_gather_params& q = B.launches[(size_t)k];
        uvrt_ctx::GatherMemo m;
        m.valid = true;
        m.first = B.first; m.count = B.tri_count; m.samples = B.samples; m.mode = B.mode; m.photons_equiv = q.photons_equiv;
        m.seed = q.seed;
        memcpy(m.from, q.from, 12);
        memcpy(m.to, q.to, 12);
        m.light_length = q.light_length;
        c->derived.gather_memo = m;
    }
    return UVRT_OK;
}

int uvrt_gather_batch_info(uvrt_ctx* c, int32_t out4[4])
{
    if (!c || !out4) return fail(UVRT_ERR_INVALID, "uvrt_gather_batch_info: null argument");
    const GatherBatch& B = c->derived.gather_batch;
    const bool have = c->have_scene && B.count > 0;
    out4[0] = have ? B.count : 0;
    out4[1] = have ? B.samples : 0;
    out4[2] = have ? B.first : 0;
    out4[3] = have ? B.tri_count : 0;
    return UVRT_OK;
}

int uvrt_read_gather_batch(uvrt_ctx* c, int32_t k, int32_t which, double* out, int32_t first, int32_t count)
{
    if (!c || !out) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_batch: null argument");
    const GatherBatch& B = c->derived.gather_batch;
    if (!c->have_scene || B.count == 0) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_batch: no batch (uvrt_gather_direct_batch)");
    if (k < 0 || k >= B.count) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_batch: k = %d outside the batch's [0, %d)", k, B.count);
    if (which != 0 && which != 1) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_batch: which must be 0 (expected) or 1 (variance), not %d", which);
    if (which == 1 && !B.var) return fail(UVRT_ERR_INVALID, "uvrt_read_gather_batch: the batch has no variance plane (uvrt_set_gather_variance)");
    if (!range_ok(out, first, count, c->T))
        return fail(UVRT_ERR_INVALID, "uvrt_read_gather_batch: range [%d,+%d) outside [0,%d)", first, count, c->T);
    char* base = (char*)(which ? B.v.p : B.e.p) + (size_t)k * (size_t)c->T * 8;
    return range_copy(c, base, 8, out, first, count, hipMemcpyDeviceToHost);
}

}  // extern "C"

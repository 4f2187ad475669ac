// uvrt_capi_free.hip -- rays with origins of their own (include/uvrt.h "free rays"): uvrt_write_free_rays,
// uvrt_generate_sweep, uvrt_seed_next_sweep, and the uvrt_extend that follows either (uvrt_extend_free.hip's kernel)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

// The scene's free records, made once per scene by the first launch that needs them (a free launch, a shadow-ray launch):
// callers that never trace such rays do not pay for them.
int make_free_records(uvrt_ctx* c)
{
    if (int rc = c->derived.free_recs.ensure(((size_t)c->npairs + (size_t)c->T + 1) * 64, true, c->stream)) return rc;
    launch_prepare_free_records(c->pairs.as<PairRec>(), c->ltris.as<LeafTri>(), c->derived.free_recs.p, c->npairs, c->T, c->stream);
    c->derived.free_recs_valid = true;
    return UVRT_OK;
}

int ensure_free_records(uvrt_ctx* c)
{
    if (c->derived.free_recs_valid) return UVRT_OK;
    // on the context's stream, behind everything outstanding; the lanes' later work waits for it (mark_fence)
    if (int rc = join_all(c)) return rc;
    if (int rc = make_free_records(c)) return rc;
    HIP_TRY(hipGetLastError());
    return mark_fence(c);
}

// ... and the current lane's {orig.x, orig.z} array, made on the lane's first free launch
static int ensure_free_buffers(uvrt_ctx* c, hipStream_t ls)
{
    Lane& L = cur_lane(c);
    if (int rc = L.oxz.ensure((size_t)std::max<int64_t>(c->capacity, 1) * 8, false, ls)) return rc;
    return ensure_free_records(c);
}

int extend_free(uvrt_ctx* c, int64_t n)
{
    if (c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "uvrt_extend: rays with origins of their own are traced in flavours 0 and 1 only "
                    "(uvrt_set_flavour %d)", c->flavour);
    if (c->record_hits) {
        if (int rc = c->hits.ensure((size_t)c->capacity * 8, false, c->stream)) return rc;
    }
    Lane& L = cur_lane(c);
    if (!L.oxz.p || !c->derived.free_recs_valid) return fail(UVRT_ERR_INVALID, "uvrt_extend: the free rays are gone (uvrt_set_scene / uvrt_resize_rays since)");
    FreeParams fp;
    fill_launch(c, fp.e, 0.0f, 0.0f);       // (force_exact: the scene's and the variant's conditions; the origins are per ray)
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls)) return rc;
    fp.e.rays = L.rays.as<float4>();
    fp.oxz = L.oxz.as<float2>();
    fp.e.hits = c->record_hits ? c->hits.as<uint2>() : nullptr;
    fp.e.counts = L.counts.as<int32_t>();
    fp.e.count_replicas = c->replicas;
    fp.e.count_stride = c->T;
    fp.e.n = n;
    fp.e.recs = c->derived.free_recs.p;
    // the grid knob of uvrt_set_variant applies; the leaf period / cache code does not (one kernel)
    const int per_cu_default = (c->cur_pipelined && c->nlanes >= 4) ? 4 : c->cur_pipelined ? 7 : 8;
    if (int rc = timed_launch(c, ls, "uvrt_extend", "the free-ray launch",
                              [&] { return launch_extend_free(fp, variant_per_cu(c->variant, per_cu_default), ls); }))
        return rc;
    L.counts_dirty = true;
    c->last.extended = c->record_hits;
    return UVRT_OK;
}

}  // namespace uvrt_impl

extern "C" {

uint32_t uvrt_seed_next_sweep(const float from[3], float light_length, uint32_t seed_prev)
{
    // work-item 0: generate.cl:13-35 at `from`, then the draw for the place on the segment
    uint32_t seed = uvrt_seed_next_mode(from, light_length, seed_prev, 0);
    (void)host_random_float(seed);
    return seed;
}

int uvrt_write_free_rays(uvrt_ctx* c, const void* rays32, int64_t n)
{
    if (!c || !rays32 || n <= 0 || n > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_write_free_rays: n must be in (0, capacity]");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_write_free_rays: no scene");
    if (int rc = set_device(c)) return rc;
    std::vector<float> packed, oxz;
    unpack_rays((const HostRay*)rays32, n, packed, &oxz);
    if (int rc = join_all(c)) return rc;
    c->lane = 0;
    c->cur_pipelined = false;
    if (int rc = ensure_free_buffers(c, c->stream)) return rc;
    Lane& L = c->lanes[0];
    HIP_TRY(hipMemcpyAsync(L.rays.p, packed.data(), (size_t)n * 16, hipMemcpyHostToDevice, c->stream));
    if (int rc = copy_sync(c, L.oxz.p, oxz.data(), (size_t)n * 8, hipMemcpyHostToDevice)) return rc;
    c->last = {n, 0, false, false, true};
    return UVRT_OK;
}

int uvrt_generate_sweep(uvrt_ctx* c, const float from[3], const float to[3], float light_length, int64_t first_gid, int64_t n)
{
    if (!c || !from || !to) return fail(UVRT_ERR_INVALID, "uvrt_generate_sweep: null argument");
    if (!c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_generate_sweep: no scene");
    if (c->seed_mode != 0)
        return fail(UVRT_ERR_INVALID, "uvrt_generate_sweep: seed mode 1 models the SEED race of generate.cl only; a sweep needs "
                    "uvrt_set_seed_mode(ctx, 0)");
    if (n < 0 || first_gid < 0 || n > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_generate_sweep: n = %lld exceeds the ray capacity %lld (uvrt_resize_rays)",
                    (long long)n, (long long)c->capacity);
    if (first_gid + n > (int64_t)INT32_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_generate_sweep: global id beyond int range (generate.cl:11)");
    if (int rc = set_device(c)) return rc;
    const uint32_t seed_prev = c->seed;
    const uint32_t seed_next = uvrt_seed_next_sweep(from, light_length, seed_prev);
    // launch lane: as uvrt_generate chooses it (ray ordering does not apply to free rays)
    if (int rc = next_launch_lane(c, true)) return rc;
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls)) return rc;
    if (int rc = ensure_free_buffers(c, ls)) return rc;
    if (int rc = lane_stream(c, &ls)) return rc;     // (again: the records' fence, when they were made just now)
    Lane& L = cur_lane(c);
    SweepParams p;
    memset(&p, 0, sizeof p);
    p.rays = L.rays.as<float4>();
    p.oxz = L.oxz.as<float2>();
    p.fx = from[0]; p.fy = from[1]; p.fz = from[2];
    p.tx = to[0]; p.ty = to[1]; p.tz = to[2];
    p.light_length = light_length;
    p.first_gid = first_gid;
    p.n = n;
    p.seed_prev = seed_prev;
    p.seed_next = seed_next;
    p.prio = c->helper_prio;
    launch_generate_sweep(p, ls);
    HIP_TRY(hipGetLastError());
    c->seed = seed_next;
    c->last = {n, first_gid, false, false, true};
    return UVRT_OK;
}

}  // extern "C"

// uvrt_capi_launch.hip -- the per-launch entry points: generate, extend, accumulate, Shade (raytracer.cpp:74-120)
// (the C ABI of include/uvrt.h over the HIP kernels; the context and its helpers are in uvrt_ctx.h)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

int hot_reset(uvrt_ctx* c, bool slab)
{
    for (auto& h : c->hot) (void)hipEventDestroy(h.ready);
    c->hot.clear();
    c->hot_slabs.clear();
    for (Lane& L : c->lanes) { L.hot_hist.release(); L.hot_list.release(); L.perm = nullptr; }
    if (!slab || c->npairs <= 128) return UVRT_OK;
    // the first slab and the lanes' scratch come with the scene: a new lamp position then costs no allocation
    c->hot_slabs.emplace_back();
    if (int rc = c->hot_slabs.back().ensure((size_t)uvrt_ctx::HOT_SLAB * (size_t)c->npairs * 4, false, c->stream)) return rc;
    for (int l = 0; l < c->nlanes || l < 3; ++l) {
        // lane 0 (uvrt_trace_batch) sets up all new lamps of a batch in one launch: room for HS_GROUPS of them where that is small
        const size_t groups = (l == 0 && (size_t)c->npairs * 4 * HS_GROUPS <= ((size_t)64 << 20)) ? (size_t)HS_GROUPS : 1;
        if (int rc = c->lanes[l].hot_hist.ensure(groups * (size_t)c->npairs * 4, true, c->stream)) return rc;
        if (int rc = c->lanes[l].hot_list.ensure(groups * ((size_t)TOP6_MAX + 1) * 4, false, c->stream)) return rc;
    }
    return UVRT_OK;
}

int hot_lookup(uvrt_ctx* c, const float lamp[3], hipStream_t s, const uint32_t** out, uvrt_ctx::HotEntry** fresh)
{
    *out = nullptr;
    *fresh = nullptr;
    if (c->have_perm) { *out = c->perm.as<uint32_t>(); return UVRT_OK; }
    if (c->hot_mode == 0 || c->npairs <= (int32_t)128 || c->root_ref >= REF_LEAF_BIT) return UVRT_OK;
    ++c->hot_clock;
    for (auto& h : c->hot)
        if (memcmp(h.lamp, lamp, 12) == 0) {
            h.stamp = c->hot_clock;
            HIP_TRY(hipStreamWaitEvent(s, h.ready, 0));      // it may have been built on another lane's stream
            *out = h.perm;
            return UVRT_OK;
        }
    uvrt_ctx::HotEntry* e = nullptr;
    if ((int)c->hot.size() < uvrt_ctx::HOT_MAX) {
        const size_t idx = c->hot.size();
        if (idx / uvrt_ctx::HOT_SLAB >= c->hot_slabs.size()) {
            c->hot_slabs.emplace_back();
            if (int rc = c->hot_slabs.back().ensure((size_t)uvrt_ctx::HOT_SLAB * (size_t)c->npairs * 4, false, s)) {
                c->hot_slabs.pop_back();
                return rc;
            }
        }
        uvrt_ctx::HotEntry ne;
        memset(&ne, 0, sizeof ne);
        ne.perm = c->hot_slabs[idx / uvrt_ctx::HOT_SLAB].as<uint32_t>() + (idx % uvrt_ctx::HOT_SLAB) * (size_t)c->npairs;
        HIP_TRY(hipEventCreateWithFlags(&ne.ready, hipEventDisableTiming));
        c->hot.push_back(ne);                 // (the vector's capacity is HOT_MAX from the start: entries never move)
        e = &c->hot.back();
    } else {          // recycle the least recently used entry: nothing in flight may still read its renumbering
        if (int rc = join_all(c)) return rc;
        HIP_TRY(hipStreamSynchronize(c->stream));
        e = &c->hot[0];
        for (auto& h : c->hot) if (h.stamp < e->stamp) e = &h;
    }
    memcpy(e->lamp, lamp, 12);
    e->stamp = c->hot_clock;
    e->gen = ++c->perm_clock;            // records prepared from the entry's previous renumbering are stale (uvrt_trace_batch's keys)
    *fresh = e;
    return UVRT_OK;
}

int hot_build(uvrt_ctx* c, uvrt_ctx::HotEntry* const* entries, const uint32_t* seed_prev, const uint32_t* seed_next, int count,
              float light_length, hipStream_t s, int lane)
{
    Lane& L = c->lanes[lane];
    for (int k0 = 0; k0 < count; k0 += HS_GROUPS) {
        const int kc = std::min(HS_GROUPS, count - k0);
        // scratch of the set-up kernels, per launch lane: visit counters (zero between uses) and the hot lists
        if (int rc = L.hot_hist.ensure((size_t)kc * (size_t)c->npairs * 4, true, s)) return rc;
        if (int rc = L.hot_list.ensure((size_t)kc * ((size_t)TOP6_MAX + 1) * 4, false, s)) return rc;
        HotSetupParams p;
        memset(&p, 0, sizeof p);
        p.pairs = c->pairs.as<PairRec>();
        p.ltris = c->ltris.as<LeafTri>();
        p.leaf_count = c->leaf_count.as<uint32_t>();
        p.root_ref = c->root_ref;
        p.light_length = light_length;
        p.seed_mode = c->seed_mode;
        // the statistics always sample global ids [0, hot_sample) of the lamp (the kernel makes its own rays), whichever
        // range of the launch this context traces
        p.n = c->hot_sample;
        p.tail_lanes = c->hot_tail;
        p.direct_bins = c->hot_direct;
        p.npairs = c->npairs;
        p.keep = (int32_t)TOP6_MAX;
        p.count = kc;
        p.hist = L.hot_hist.as<uint32_t>();
        p.hot_list = L.hot_list.as<uint32_t>();
        for (int k = 0; k < kc; ++k) {
            const uvrt_ctx::HotEntry* e = entries[k0 + k];
            p.perm[k] = e->perm;
            p.lx[k] = e->lamp[0]; p.ly[k] = e->lamp[1]; p.lz[k] = e->lamp[2];
            p.seed_prev[k] = seed_prev[k0 + k];
            p.seed_next[k] = seed_next[k0 + k];
        }
        launch_hot_setup(p, s);
        HIP_TRY(hipGetLastError());
        for (int k = 0; k < kc; ++k) HIP_TRY(hipEventRecord(entries[k0 + k]->ready, s));
    }
    return UVRT_OK;
}

int launch_perm(uvrt_ctx* c, const float lamp[3], float light_length, uint32_t seed_prev, uint32_t seed_next,
                hipStream_t s, int lane, const uint32_t** out)
{
    uvrt_ctx::HotEntry* fresh = nullptr;
    if (int rc = hot_lookup(c, lamp, s, out, &fresh)) return rc;
    if (!fresh) return UVRT_OK;
    if (int rc = hot_build(c, &fresh, &seed_prev, &seed_next, 1, light_length, s, lane)) return rc;
    *out = fresh->perm;
    return UVRT_OK;
}

}  // namespace uvrt_impl

extern "C" {

uint32_t uvrt_seed_next(const float lp[3], float light_length, uint32_t seed_prev)
{
    return uvrt_seed_next_mode(lp, light_length, seed_prev, 0);
}

uint32_t uvrt_seed_next_mode(const float lp[3], float light_length, uint32_t seed_prev, int32_t seed_mode)
{
    // work-item 0 of cl/generate.cl:13-39; the ray itself is not needed, only the RNG state
    float acc = (float)(0 * 17 + 1);
    acc = acc + lp[0] * 13.0f;
    acc = acc + lp[1] * 7.0f;
    acc = acc + lp[2] * 11.0f;
    acc = acc + (float)(seed_prev >> 15);
    uint32_t seed = host_wang_hash((seed_mode == 1 && acc < 0.0f) ? 0u : (uint32_t)(int64_t)acc);
    (void)light_length;
    (void)host_random_float(seed);   // origin.y
    (void)host_random_float(seed);   // diry
    double x = (double)(host_random_float(seed) * 2.0f - 1.0f);
    double y = (double)(host_random_float(seed) * 2.0f - 1.0f);
    while (x * x + y * y > 1.0) {
        x = (double)(host_random_float(seed) * 2.0f - 1.0f);
        y = (double)(host_random_float(seed) * 2.0f - 1.0f);
    }
    return seed;
}

int uvrt_generate(uvrt_ctx* c, const float lp[3], float light_length, int64_t first_gid, int64_t n)
{
    if (!c || !lp) return fail(UVRT_ERR_INVALID, "uvrt_generate: null argument");
    if (n < 0 || first_gid < 0 || n > c->capacity)
        return fail(UVRT_ERR_INVALID, "uvrt_generate: n = %lld exceeds the ray capacity %lld (uvrt_resize_rays)",
                    (long long)n, (long long)c->capacity);
    if (first_gid + n > (int64_t)INT32_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_generate: global id beyond int range (generate.cl:11)");
    if (int rc = set_device(c)) return rc;

    const uint32_t seed_prev = c->seed;
    const uint32_t seed_next = uvrt_seed_next_mode(lp, light_length, seed_prev, c->seed_mode);

    int bits = c->sort_bits < 0 ? auto_sort_bits(n) : c->sort_bits;
    if (bits > 20) bits = 20;
    // launch lane: alternate between the two streams / buffer sets when nothing stands against it (ray ordering does)
    if (int rc = next_launch_lane(c, bits == 0)) return rc;
    Lane& L = cur_lane(c);
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls)) return rc;
    GenParams p;
    memset(&p, 0, sizeof p);
    p.rays = L.rays.as<float4>();
    p.lx = lp[0]; p.ly = lp[1]; p.lz = lp[2];
    p.light_length = light_length;
    p.first_gid = first_gid;
    p.n = n;
    p.seed_prev = seed_prev;
    p.seed_next = seed_next;
    p.seed_mode = c->seed_mode;
    if (bits > 0 && n > 0) {
        const int32_t nbins = 1 << bits;
        if (c->hist_bins < nbins) {
            int rc;
            HIP_TRY(hipStreamSynchronize(c->stream));
            c->hist.release();
            c->bin_start.release();
            if ((rc = c->hist.ensure((size_t)nbins * 4, true, c->stream))) return rc;
            if ((rc = c->bin_start.ensure((size_t)nbins * 4, true, c->stream))) return rc;
            c->hist_bins = nbins;
        }
        p.keyrank = c->keyrank.as<uint2>();
        p.hist = c->hist.as<uint32_t>();
        split_bits(bits, p.bits_phi, p.bits_y, p.bits_o);
    }
    if (c->npairs > 0) {   // extend's per-launch records ride along in the same launch
        p.prep_pairs = c->pairs.as<PairRec>();
        p.prep_recs = L.recs.as<float4>();
        // launches too small to repay the statistics keep the breadth-first order
        const uint32_t* pm = c->have_perm ? c->perm.as<uint32_t>() : nullptr;
        if (!pm && n >= 16384)
            if (int rc = launch_perm(c, lp, light_length, seed_prev, seed_next, ls, c->lane, &pm)) return rc;
        L.perm = pm;
        p.prep_perm = pm;
        p.prep_npairs = c->npairs;
    }
    p.prio = c->helper_prio;
    launch_generate(p, ls);
    HIP_TRY(hipGetLastError());
    L.recs_tag = {p.prep_recs != nullptr, lp[0], lp[2]};
    if (p.keyrank) {     // (ray ordering keeps the launch on lane 0)
        launch_scan_bins(c->hist.as<uint32_t>(), c->bin_start.as<uint32_t>(), 1 << bits, c->stream);
        launch_scatter(L.rays.as<float4>(), c->keyrank.as<uint2>(), c->bin_start.as<uint32_t>(),
                       c->sorted.as<float4>(), c->order.as<uint32_t>(), n, c->stream);
        HIP_TRY(hipGetLastError());
    }
    c->seed = seed_next;
    c->last = {n, first_gid, p.keyrank != nullptr, false, false};
    c->ox = lp[0];
    c->oz = lp[2];
    return UVRT_OK;
}

int uvrt_extend(uvrt_ctx* c, int64_t n)
{
    if (!c || !c->have_scene) return fail(UVRT_ERR_INVALID, "uvrt_extend: no scene");
    if (c->last.n < 0 || n != c->last.n)
        return fail(UVRT_ERR_INVALID, "uvrt_extend: n = %lld does not match the last generate (%lld)",
                    (long long)n, (long long)c->last.n);
    if (int rc = set_device(c)) return rc;
    if (c->last.free_rays) return extend_free(c, n);      // rays with origins of their own: the free-origin kernel, whatever the walk / ordering knobs say
    if (c->record_hits) {
        if (int rc = c->hits.ensure((size_t)c->capacity * 8, false, c->stream)) return rc;
    }
    Lane& L = cur_lane(c);
    ExtendParams p;
    fill_launch(c, p, c->ox, c->oz);
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls)) return rc;
    p.rays = c->last.sorted ? c->sorted.as<float4>() : L.rays.as<float4>();
    p.order = c->last.sorted ? c->order.as<uint32_t>() : nullptr;
    p.hits = c->record_hits ? c->hits.as<uint2>() : nullptr;
    p.counts = L.counts.as<int32_t>();
    p.count_replicas = c->replicas;
    p.count_stride = c->T;
    p.n = n;
    p.recs = L.recs.p;
    p.perm = c->have_perm ? c->perm.as<uint32_t>() : L.perm;
    p.recs_prepared = L.recs_tag.matches(c->ox, c->oz) ? 1 : 0;
    if (c->wide && c->nquads > 0) {
        // the opt-in 4-wide walk: its per-launch records are (re)made here when the lane's are for another lamp
        const bool new_recs4 = !L.recs4.p;
        if (new_recs4)
            if (int rc = L.recs4.ensure(((size_t)2 * c->nquads + (size_t)c->T + 1) * 64, true, ls)) return rc;
        p.recs4 = L.recs4.p;
        p.nquads = c->nquads;
        p.top_quads = c->top_quads;
        p.refill_min = 8;
        if (int rc = timed_launch(c, ls, "uvrt_extend", "the 4-wide kernel", [&] {
                if (new_recs4) {
                    launch_prepare_leaves6(c->ltris.as<LeafTri>(), L.recs4.p, 2 * c->nquads, c->T, ls);
                    L.recs4_tag.valid = false;
                }
                if (!L.recs4_tag.matches(c->ox, c->oz)) {
                    launch_prepare_launch4(c->quads.as<QuadRec>(), L.recs4.p, c->ox, c->oz, c->nquads, ls);
                    L.recs4_tag = {true, c->ox, c->oz};
                }
                return launch_extend4(p, 7, ls);
            }))
            return rc;
    } else {
        // default grid: 8 workgroups per CU on one stream (20 KB of LDS each: eight fit a CU); 7 when launches are
        // pipelined over several streams -- the free slot per CU lets the first workgroups of the next launch and the
        // small kernels around it (generate, accumulate, replay) run at once instead of queueing behind persistent waves
        // (profiles/r02/r02_experiments.txt); with four launch lanes 4 per CU
        const int per_cu_default = (c->cur_pipelined && c->nlanes >= 4) ? 4 : c->cur_pipelined ? 7 : 8;
        if (int rc = timed_launch(c, ls, "uvrt_extend", "the launch", [&] {
                return launch_extend6(p, variant_code6(c->variant), variant_per_cu(c->variant, per_cu_default), c->helper_prio, ls);
            }))
            return rc;
    }
    L.counts_dirty = true;
    c->last.extended = c->record_hits;
    return UVRT_OK;
}

int uvrt_accumulate(uvrt_ctx* c, float time_step, int32_t tri_count)
{
    if (!c || !c->have_scene || tri_count < 0 || tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_accumulate: bad tri_count");
    if (int rc = set_device(c)) return rc;       // (an earlier deferred accumulate goes first)
    // the maps are updated in launch order: wait for whatever the other lane has enqueued so far
    // (its accumulate and shade), not for this lane's successor
    if (int rc = order_after_previous(c)) return rc;
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls, true)) return rc;
    if (tri_count == c->T && c->T > 0) {
        // deferred: the ordering is enqueued, the launch waits for the next call -- a uvrt_shade takes it along in one
        // kernel (uvrt_ctx.h PendingAcc), anything else launches it first
        c->pend.valid = true;
        c->pend.lane = c->lane;
        c->pend.time_step = time_step;
        cur_lane(c).counts_dirty = false;
        return UVRT_OK;
    }
    launch_accumulate(c->photon_map.as<double>(), c->max_map.as<double>(), cur_lane(c).counts.as<int32_t>(),
                      c->replicas, c->T, time_step, tri_count, c->helper_prio, ls);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

int uvrt_compute_dosage(uvrt_ctx* c, int32_t which, int32_t photons_per_light, float scaled_power,
                        int32_t tri_count)
{
    if (!c || !c->have_scene || tri_count < 0 || tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_compute_dosage: bad tri_count");
    if (which != UVRT_MAP_SUM && which != UVRT_MAP_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_compute_dosage: which_map must be 0 or 1");
    if (int rc = set_device(c)) return rc;
    const double* map = which == UVRT_MAP_SUM ? c->photon_map.as<double>() : c->max_map.as<double>();
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls, true)) return rc;
    launch_compute_dosage(map, c->dosage.as<float>(), c->area.as<float>(), photons_per_light,
                          scaled_power, tri_count, ls);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

int uvrt_dosage_to_color(uvrt_ctx* c, float min_value, int32_t threshold_view, int32_t tri_count)
{
    if (!c || !c->have_scene || tri_count < 0 || tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_dosage_to_color: bad tri_count");
    if (int rc = set_device(c)) return rc;
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls, true)) return rc;
    launch_dosage_to_color(c->dosage.as<float>(), c->color.as<float>(), min_value, threshold_view,
                           tri_count, ls);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

int uvrt_shade(uvrt_ctx* c, int32_t which, int32_t photons_per_light, float scaled_power, float min_value,
               int32_t threshold_view, int32_t tri_count)
{
    if (!c || !c->have_scene || tri_count < 0 || tri_count > c->T)
        return fail(UVRT_ERR_INVALID, "uvrt_shade: bad tri_count");
    if (which != UVRT_MAP_SUM && which != UVRT_MAP_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_shade: which_map must be 0 or 1");
    if (c->pend.valid && c->pend.lane == c->lane && tri_count == c->T) {
        // the launch's accumulate is still pending on this lane: accumulate + computeDosage + dosageToColor in one kernel
        if (int rc = set_device_only(c)) return rc;
        hipStream_t fs;
        if (int rc = lane_stream(c, &fs, true)) return rc;
        c->pend.valid = false;
        launch_accumulate_shade(c->photon_map.as<double>(), c->max_map.as<double>(), cur_lane(c).counts.as<int32_t>(), c->replicas,
                                c->T, c->pend.time_step, c->dosage.as<float>(), c->area.as<float>(), c->color.as<float>(),
                                which == UVRT_MAP_SUM ? 0 : 1, photons_per_light, scaled_power, min_value, threshold_view,
                                tri_count, c->helper_prio, fs);
        HIP_TRY(hipGetLastError());
        return UVRT_OK;
    }
    if (int rc = set_device(c)) return rc;
    const double* map = which == UVRT_MAP_SUM ? c->photon_map.as<double>() : c->max_map.as<double>();
    hipStream_t ls;
    if (int rc = lane_stream(c, &ls, true)) return rc;
    launch_shade(map, c->dosage.as<float>(), c->area.as<float>(), c->color.as<float>(), photons_per_light,
                 scaled_power, min_value, threshold_view, tri_count, c->helper_prio, ls);
    HIP_TRY(hipGetLastError());
    return UVRT_OK;
}

int uvrt_advance_seed(uvrt_ctx* c, const float lp[3], float light_length)
{
    if (!c || !lp) return fail(UVRT_ERR_INVALID, "uvrt_advance_seed: null argument");
    c->seed = uvrt_seed_next_mode(lp, light_length, c->seed, c->seed_mode);
    return UVRT_OK;
}

}  // extern "C"

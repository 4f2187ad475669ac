// uvrt_capi_batch.hip -- batched tracing: several launches in one go, one count plane per launch
// (the C ABI of include/uvrt.h over the HIP kernels; the context and its helpers are in uvrt_ctx.h, the host-only plan of a
// batch in uvrt_batch_plan.h)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

static BatchKnobs batch_knobs(const uvrt_ctx* c)
{
    BatchKnobs kn = {};
    kn.seed = c->seed; kn.seed_mode = c->seed_mode; kn.T = c->T; kn.replicas = c->replicas;
    kn.may_dedupe = c->dedupe && variant_code6(c->variant) == 1;
#ifdef UVRT_DEV_VARIANTS
    kn.may_dedupe = kn.may_dedupe && c->probe_skip_generate <= 0;
#endif
    kn.dedupe_classes = c->dedupe_classes; kn.dedupe_class_replicas = c->dedupe_class_replicas;
    kn.dedupe_class_bytes = c->dedupe_class_bytes; kn.dedupe_periodic = c->dedupe_periodic;
    kn.dedupe_chunk_bytes = c->dedupe_chunk_bytes; kn.batch_chunk_bytes = c->batch_chunk_bytes; kn.dedupe_strip = c->dedupe_strip;
    return kn;
}

// One call's way from its plan to the streams: what provision_batch, the three chunk emitters and commit_batch share.
struct BatchRun {
    uvrt_ctx* c;
    int set;                            // the buffer set the batch goes into, S = c->bs[set]
    uvrt_ctx::BatchSet& S;
    const BatchPlan& P;
    const char* who;                    // the caller, for the error texts
    float light_length;
    int64_t first_gid, n;
    const uint32_t* gperm[MAX_BATCH];   // per lamp column: the renumbering of its records (provision_batch), and its stamp
    uint64_t ggen[MAX_BATCH];
    bool lane_waited[uvrt_ctx::MAXL];   // the lane has waited for the set's last replay
    int per_cu;
    int64_t traced;                     // rays handed to k_extend6 with their count known here; the deduped chunks' counts stay on the device
    size_t dd_used;                     // deduped chunks enqueued
};

// The renumberings of the columns' records -- the caller's, or a hot-record set-up: lamps the context has not seen get theirs
// in ONE launch on the context's stream -- and whether some column's record array holds something else.
static int provision_records(BatchRun& r, bool* recs_stale)
{
    uvrt_ctx* c = r.c;
    const BatchPlan& P = r.P;
    uvrt_ctx::HotEntry* fresh[MAX_BATCH];
    uint32_t fresh_prev[MAX_BATCH], fresh_next[MAX_BATCH];
    int nfresh = 0;
    for (int g = 0; g < P.ngroups; ++g) {
        r.gperm[g] = c->have_perm ? c->perm.as<uint32_t>() : nullptr;
        bool is_fresh = false;
        if (!r.gperm[g] && (int64_t)P.gsize[g] * r.n >= 16384) {
            const int ph = P.gfirst[g];      // the group's first launch lends its lamp and seeds to the statistics
            const float gl[3] = {P.gp.lx[ph], P.gp.ly[ph], P.gp.lz[ph]};
            uvrt_ctx::HotEntry* e = nullptr;
            if (int rcp = hot_lookup(c, gl, c->stream, &r.gperm[g], &e)) return rcp;
            if (e) {
                r.gperm[g] = e->perm;
                fresh[nfresh] = e; fresh_prev[nfresh] = P.gp.seed_prev[ph]; fresh_next[nfresh] = P.gp.seed_next[ph];
                ++nfresh;
                is_fresh = true;
            }
        }
        r.ggen[g] = perm_generation(c, r.gperm[g]);
        if (g >= (int)c->b_recs_key.size() || !c->b_recs_key[g].holds(P.gx[g], P.gz[g], r.gperm[g], r.ggen[g]) || is_fresh) {
            *recs_stale = true;
            if (g < (int)c->b_recs_key.size()) c->b_recs_key[g].tag.valid = false;
        }
    }
    if (nfresh > 0)
        if (int rcb = hot_build(c, fresh, fresh_prev, fresh_next, nfresh, r.light_length, c->stream, 0)) return rcb;
    return UVRT_OK;
}

// The batch goes into the buffer set the previous batch did NOT use: its lanes start at once -- in the drain of
// the previous batch, while that one is still being folded / reduced / replayed on the context's stream -- and
// only wait for the set's last replay (free_ev), which is two batches back.  Anything that has to touch memory
// the lanes may still read (growing a buffer, new per-launch records) first waits for everything.
static int provision_batch(BatchRun& r, int count)
{
    uvrt_ctx* c = r.c;
    uvrt_ctx::BatchSet& S = r.S;
    const BatchPlan& P = r.P;
    int rc;
    const int64_t n_pad = P.n_pad;
    // full planes are allocated for the context's replica count: R only shrinks the part of it that is used
    const size_t plane_alloc = (size_t)c->replicas * (size_t)c->T;
    const size_t planes_bytes = (size_t)count * plane_alloc * 4 + (size_t)P.class_cap * P.plane_ints * 4;
    // growing a buffer needs the device idle (hipFree / hipMalloc); new per-launch records only need the context's stream
    // ordered after the lanes' earlier work -- no host synchronisation, so a new lamp position costs its kernels only
    bool dd_scratch_short = false;      // (every lane a chunk may run on: 0 without pipelining, else 1..batch_lanes)
    for (int l = 0; l <= c->batch_lanes; ++l)
        dd_scratch_short = dd_scratch_short || c->lanes[l].dd_tmp.bytes < P.dd_tmp_bytes || c->lanes[l].dd_blocks.bytes < P.dd_block_bytes;
    const bool need_alloc = S.rays.bytes < (size_t)count * (size_t)n_pad * 16 || S.planes.bytes < planes_bytes ||
                            S.folded.bytes < (size_t)count * (size_t)c->T * 4 || (int)c->b_recs.size() < P.ngroups || !S.free_ev ||
                            S.oxz.bytes < (size_t)P.nsweeps * (size_t)n_pad * 8 || (P.nsweeps > 0 && !c->derived.free_recs_valid) ||
                            (P.dd_chunks > 0 && (S.masks.bytes < (size_t)count * (size_t)n_pad * 4 || S.dd_counts.bytes < P.dd_chunks * 8 ||
                                                 dd_scratch_short));
    bool recs_stale = false;
    if ((rc = provision_records(r, &recs_stale))) return rc;
    if (need_alloc || recs_stale) {
        if (int rcj = join_all(c)) return rcj;
    }
    if (need_alloc) {
        HIP_TRY(hipStreamSynchronize(c->stream));
        if (!S.free_ev) HIP_TRY(hipEventCreateWithFlags(&S.free_ev, hipEventDisableTiming));
        const bool grown = S.planes.bytes < planes_bytes || S.folded.bytes < (size_t)count * (size_t)c->T * 4;
        if ((rc = S.rays.ensure((size_t)count * (size_t)n_pad * 16, false, c->stream))) return rc;
        if ((rc = S.planes.ensure(planes_bytes, true, c->stream))) return rc;
        if ((rc = S.folded.ensure((size_t)count * (size_t)c->T * 4, true, c->stream))) return rc;
        if ((rc = S.oxz.ensure((size_t)P.nsweeps * (size_t)n_pad * 8, false, c->stream))) return rc;      // (8 B of origin per photon of a sweep)
        if (grown) HIP_TRY(hipEventRecord(S.free_ev, c->stream));      // the zero fill is the set's "last replay"
        while ((int)c->b_recs.size() < P.ngroups) {
            DevBuf b;
            if ((rc = b.ensure(((size_t)c->npairs + (size_t)c->T + 1) * 64, true, c->stream))) return rc;
            launch_prepare_leaves6(c->ltris.as<LeafTri>(), b.p, c->npairs, c->T, c->stream);
            c->b_recs.push_back(std::move(b));
        }
        c->b_recs_key.resize(c->b_recs.size());
        for (int l = 1; l <= c->batch_lanes; ++l)
            if ((rc = c->lanes[l].ovf.ensure(side_ovf_bytes(c), false, c->stream))) return rc;
        if (P.dd_chunks > 0) {      // the deduped chunks' masks and counts, and every lane's scratch between the generate passes
            if ((rc = S.masks.ensure((size_t)count * (size_t)n_pad * 4, false, c->stream))) return rc;
            // (not zeroed: a chunk's generate runs on its lane BEFORE the lane waits for this stream, and writes its count;
            //  the chunks' ray counts first, their deposit counts behind them)
            if ((rc = S.dd_counts.ensure(P.dd_chunks * 8, false, c->stream))) return rc;
            // (dd_blocks zeroed: k_dedupe_mark adds its owners to it and k_dedupe_write leaves it zero again.  A chunk's generate
            //  does not wait for this stream, so the zero fill is waited for here, where a buffer has grown)
            for (int l = 0; l <= c->batch_lanes; ++l) {
                if ((rc = c->lanes[l].dd_tmp.ensure(P.dd_tmp_bytes, false, c->stream))) return rc;
                if ((rc = c->lanes[l].dd_blocks.ensure(P.dd_block_bytes, true, c->stream))) return rc;
            }
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    if (need_alloc || recs_stale) {
        // per-launch records of the lamp columns whose array holds something else
        for (int g = 0; g < P.ngroups; ++g) {
            uvrt_ctx::RecsKey& key = c->b_recs_key[g];
            if (key.holds(P.gx[g], P.gz[g], r.gperm[g], r.ggen[g])) continue;
            launch_prepare_launch6(c->pairs.as<PairRec>(), c->b_recs[g].p, P.gx[g], P.gz[g], c->npairs, r.gperm[g], c->helper_prio, c->stream);
            key = {{true, P.gx[g], P.gz[g]}, r.gperm[g], r.ggen[g]};
        }
        // the scene's free records, on first use (the lanes are joined above, the fence below covers them)
        if (P.nsweeps > 0 && !c->derived.free_recs_valid)
            if ((rc = make_free_records(c))) return rc;
        HIP_TRY(hipGetLastError());
        if (int rcf = mark_fence(c)) return rcf;         // the lanes' next work waits for the records
    }
    return UVRT_OK;
}

// The lane of the next chunk.  Two SIDE lanes in turn: the context's own stream carries the fold / reduce / replay of the
// previous batch, which a chunk enqueued there would have to wait for.  The chunk's rays depend on nothing but their
// buffer: generate goes to the lane's stream (*ls) BEFORE the lane waits for the context's stream (lane_stream: new
// records, a hot-record set-up), so it runs beside them.
static int next_chunk_lane(BatchRun& r, hipStream_t* ls)
{
    uvrt_ctx* c = r.c;
    c->lane = c->pipeline ? 1 + (int)(c->b_chunks++ % (uint64_t)c->batch_lanes) : 0;
    *ls = stream_of(c, c->lane);
    if (c->lane != 0) cur_lane(c).used = true;
    if (!r.lane_waited[c->lane]) {      // the set's previous occupant has been replayed (two batches back)
        HIP_TRY(hipStreamWaitEvent(*ls, r.S.free_ev, 0));
        r.lane_waited[c->lane] = true;
    }
    return UVRT_OK;
}
// what the fused extend of a chunk of kc planes from physical plane ph0 on gets besides its rays and records
static void set_planes(const BatchRun& r, ExtendParams& p, int ph0, int kc)
{
    p.counts = r.S.planes.as<int32_t>() + (size_t)ph0 * r.P.plane_ints;
    p.count_replicas = r.P.R;
    p.count_stride = r.c->T;
    p.n = (int64_t)kc * r.P.n_pad;
    p.plane_batches = (uint32_t)(r.P.n_pad / 64);
    p.plane_n = (uint32_t)r.n;
    p.plane_stride = (uint32_t)r.P.plane_ints;
}

// what a chunk's generate gets of a dedupe group: the piece's group, classes and period table, the gids [g0, g0 + gn) of the
// call's range, the lane's scratch and the key tiles of the mark pass; the caller adds where the rays and counts go
static void fill_dedupe_chunk(const uvrt_ctx* c, GenDedupeParams& dq, const Piece& pc, int64_t g0, int64_t gn, const Lane& L, float light_length)
{
    memset(&dq, 0, sizeof dq);
    dq.g = pc.G;
    dq.cls = pc.cls;
    dq.per = pc.per;
    dq.tmp = L.dd_tmp.as<uint32_t>();
    dq.g0 = g0;
    dq.gn = gn;
    dq.block_counts = L.dd_blocks.as<uint32_t>();
    mark_tiles(c->dedupe_strip, dq);
    dq.light_length = light_length;
    dq.prio = c->helper_prio;
}
// the lamps and seeds of the kc planes from physical plane ph0 on; of the kc sweeps from sweep k0 on
static void copy_stops(GenBatchParams& gq, const BatchPlan& P, int ph0, int kc)
{
    for (int j = 0; j < kc; ++j) {
        gq.lx[j] = P.gp.lx[ph0 + j]; gq.ly[j] = P.gp.ly[ph0 + j]; gq.lz[j] = P.gp.lz[ph0 + j];
        gq.seed_prev[j] = P.gp.seed_prev[ph0 + j]; gq.seed_next[j] = P.gp.seed_next[ph0 + j];
    }
}
static void copy_sweeps(SweepBatchParams& sq, const BatchPlan& P, int k0, int kc)
{
    for (int j = 0; j < kc; ++j) {
        sq.fx[j] = P.sp.fx[k0 + j]; sq.fy[j] = P.sp.fy[k0 + j]; sq.fz[j] = P.sp.fz[k0 + j];
        sq.tx[j] = P.sp.tx[k0 + j]; sq.ty[j] = P.sp.ty[k0 + j]; sq.tz[j] = P.sp.tz[k0 + j];
        sq.seed_prev[j] = P.sp.seed_prev[k0 + j]; sq.seed_next[j] = P.sp.seed_next[k0 + j];
    }
}

// A chunk of a dedupe group: the gids [g0, g0 + gn) of the call's range across all the piece's launches.  Whether an
// occurrence is an owner is decided over the whole call's range, a chunk only says where the owner's ray is generated.
static int enqueue_dedupe_chunk(BatchRun& r, const Piece& pc, int64_t g0, int64_t gn)
{
    uvrt_ctx* c = r.c;
    const BatchPlan& P = r.P;
    const int g = pc.g, ph0 = P.gfirst[g] + pc.k0;
    hipStream_t ls;
    if (int rcl = next_chunk_lane(r, &ls)) return rcl;
    const size_t at = (size_t)ph0 * (size_t)P.n_pad + (size_t)pc.kc * (size_t)g0;
    GenDedupeParams dq;
    fill_dedupe_chunk(c, dq, pc, r.first_gid + g0, gn, cur_lane(c), r.light_length);
    dq.rays = r.S.rays.as<float4>() + at;
    dq.masks = r.S.masks.as<uint32_t>() + at;
    dq.total = r.S.dd_counts.as<uint32_t>() + r.dd_used;
    dq.deposits = r.S.dd_counts.as<uint32_t>() + P.dd_chunks + r.dd_used++;
    launch_generate_dedupe(dq, ls);
    if (int rcl = lane_stream(c, &ls)) return rcl;      // extend: after the fence
    ExtendParams p;
    fill_launch(c, p, P.gx[g], P.gz[g]);
    p.rays = dq.rays;
    p.masks = dq.masks;
    p.n_dev = dq.total;
    p.counts = r.S.planes.as<int32_t>() + (size_t)ph0 * P.plane_ints;
    p.count_replicas = P.R;
    p.count_stride = c->T;
    p.n = (int64_t)pc.kc * gn;
    p.plane_stride = (uint32_t)P.plane_ints;
    p.cls_replicas = pc.cls.count > 0 ? P.cls_repl : 0;      // (0: the chunk's words are its masks)
    p.recs = c->b_recs[g].p;
    p.perm = r.gperm[g];
    p.recs_prepared = 1;
    return timed_launch(c, ls, r.who, "the stops' launch", [&] { return launch_extend6_dedupe(p, variant_code6(c->variant), r.per_cu, ls); });
}

// A chunk of kc launches of column g traced as they are, from physical plane ph0 on: generate + fused extend on one launch
// lane, chunks alternating over the lanes; the next chunk's generate and first waves run in the drain of the previous one.
static int enqueue_stop_chunk(BatchRun& r, int g, int ph0, int kc)
{
    uvrt_ctx* c = r.c;
    const BatchPlan& P = r.P;
    r.traced += (int64_t)kc * r.n;
    hipStream_t ls;
    if (int rcl = next_chunk_lane(r, &ls)) return rcl;
    GenBatchParams gq;
    memset(&gq, 0, sizeof gq);
    gq.rays = r.S.rays.as<float4>() + (size_t)ph0 * (size_t)P.n_pad;
    gq.n_pad = P.n_pad;
    gq.first_gid = r.first_gid;
    gq.n = r.n;
    gq.light_length = r.light_length;
    gq.seed_mode = c->seed_mode;
    gq.count = kc;
    gq.prio = c->helper_prio;
    copy_stops(gq, P, ph0, kc);
#ifdef UVRT_DEV_VARIANTS
    if (!(c->probe_skip_generate > 0 && c->probe_batches >= c->probe_skip_generate))
#endif
    launch_generate_batch(gq, ls);
    if (int rcl = lane_stream(c, &ls)) return rcl;      // extend: after the fence
    ExtendParams p;
    fill_launch(c, p, P.gx[g], P.gz[g]);
    p.rays = gq.rays;
    set_planes(r, p, ph0, kc);
    p.recs = c->b_recs[g].p;
    p.perm = r.gperm[g];
    p.recs_prepared = 1;
    return timed_launch(c, ls, r.who, "the stops' launch", [&] { return launch_extend6(p, variant_code6(c->variant), r.per_cu, c->helper_prio, ls); });
}

// A chunk of kc sweeps from sweep k0 on.  The sweeps are one further group (the free records are the scene's, whatever the
// segment), in chunks of as many bytes -- 16 B of ray plus 8 B of origin per photon -- over the same lanes in the same rotation.
static int enqueue_sweep_chunk(BatchRun& r, int k0, int kc)
{
    uvrt_ctx* c = r.c;
    const BatchPlan& P = r.P;
    const int ph0 = P.nstops + k0;
    hipStream_t ls;
    if (int rcl = next_chunk_lane(r, &ls)) return rcl;
    SweepBatchParams sq;
    memset(&sq, 0, sizeof sq);
    sq.rays = r.S.rays.as<float4>() + (size_t)ph0 * (size_t)P.n_pad;
    sq.oxz = r.S.oxz.as<float2>() + (size_t)k0 * (size_t)P.n_pad;
    sq.n_pad = P.n_pad;
    sq.first_gid = r.first_gid;
    sq.n = r.n;
    sq.light_length = r.light_length;
    sq.count = kc;
    sq.prio = c->helper_prio;
    copy_sweeps(sq, P, k0, kc);
#ifdef UVRT_DEV_VARIANTS
    if (!(c->probe_skip_generate > 0 && c->probe_batches >= c->probe_skip_generate))
#endif
    launch_generate_sweep_batch(sq, ls);
    if (int rcl = lane_stream(c, &ls)) return rcl;      // extend: after the fence
    FreeParams fp;
    fill_launch(c, fp.e, 0.0f, 0.0f);       // (force_exact: the scene's and the variant's conditions; the origins are per ray)
    fp.e.rays = sq.rays;
    fp.oxz = sq.oxz;
    set_planes(r, fp.e, ph0, kc);
    fp.e.recs = c->derived.free_recs.p;
    return timed_launch(c, ls, r.who, "the free-ray launch", [&] { return launch_extend_free_planes(fp, r.per_cu, ls); });
}

// the traced batch becomes the context's: the SEED chain, the set, the planes' layout and what the read-backs need
static void commit_batch(BatchRun& r, int32_t count)
{
    uvrt_ctx* c = r.c;
    const BatchPlan& P = r.P;
    c->seed = P.seed_after;
    c->lane = 0;
    c->cur_pipelined = false;
    c->last = {};                        // the per-launch generate/extend pairing starts afresh
    c->b_set = r.set;
    c->b_repl = P.R;
    c->b_count = count;
    c->b_n = r.n;
    c->b_npad = P.n_pad;
    c->b_is_folded = false;
    c->b_traced_known = r.traced;
    c->b_traced_chunks = (int32_t)r.dd_used;
    c->b_ncls = P.total_cls;
    c->b_cls_repl = P.cls_repl;
    for (const Piece& pc : P.pieces)
        for (int i = 0; i < pc.ncls; ++i) c->b_cls_launches[pc.cls_base + i] = (uint64_t)pc.cls.mask[i] << (P.gfirst[pc.g] + pc.k0);
    memcpy(c->b_phys, P.phys, sizeof(int32_t) * (size_t)count);
}

// uvrt_trace_batch and uvrt_trace_batch_launches (`who` names the caller in the error texts): generate + extend for `count`
// launches, stops grouped by lamp column and traced by k_extend6, sweeps as one further group traced by the plane-aware
// k_extend_free.  The plan (uvrt_batch_plan.h), the buffers and records, the chunks piece by piece, the commit.
static int trace_launches(uvrt_ctx* c, const uvrt_launch* launches, float light_length, int32_t count, int64_t first_gid,
                          int64_t n, const char* who)
{
    if (!c || !launches || !c->have_scene) return fail(UVRT_ERR_INVALID, "%s: null argument or no scene", who);
    if (c->b_count > 0) return fail(UVRT_ERR_INVALID, "%s: the previous batch has not been replayed (uvrt_replay_batch)", who);
    if (c->record_hits || c->sort_bits != 0)
        return fail(UVRT_ERR_INVALID, "%s: per-ray hit records and ray ordering are per-launch features", who);
    BatchPlan P;
    const char* why = nullptr;
    if (int rc = plan_batch(batch_knobs(c), launches, light_length, count, first_gid, n, P, &why)) return fail(rc, "%s: %s", who, why);
    if (P.nsweeps > 0 && c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "%s: rays with origins of their own are traced in flavours 0 and 1 only "
                    "(uvrt_set_flavour %d)", who, c->flavour);
    if (int rc = set_device(c)) return rc;
    const int set = c->b_set ^ 1;
    BatchRun r = {c, set, c->bs[set], P, who, light_length, first_gid, n, {}, {}, {}, variant_per_cu(c->variant, c->pipeline ? 7 : 8), 0, 0};
    if (int rc = provision_batch(r, count)) return rc;
    // every error return below leaves the launch-lane rotation as it found it
    struct LaneGuard {
        uvrt_ctx* c; int lane; uint64_t chunks; bool armed;
        ~LaneGuard() { if (armed) { c->lane = lane; c->b_chunks = chunks; } }
    } guard{c, c->lane, c->b_chunks, true};
    for (const Piece& pc : P.pieces) {
        if (pc.dd) {
            for (int64_t g0 = 0; g0 < n; g0 += pc.chunk_gids)
                if (int rc = enqueue_dedupe_chunk(r, pc, g0, std::min(pc.chunk_gids, n - g0))) return rc;
            continue;
        }
        for (int k0 = pc.k0; k0 < pc.k0 + pc.kc; k0 += P.per_chunk)
            if (int rc = enqueue_stop_chunk(r, pc.g, P.gfirst[pc.g] + k0, std::min(P.per_chunk, pc.k0 + pc.kc - k0))) return rc;
    }
    for (int k0 = 0; k0 < P.nsweeps; k0 += P.per_sweep_chunk)
        if (int rc = enqueue_sweep_chunk(r, k0, std::min(P.per_sweep_chunk, P.nsweeps - k0))) return rc;
#ifdef UVRT_DEV_VARIANTS
    ++c->probe_batches;
#endif
    guard.armed = false;
    commit_batch(r, count);
    return UVRT_OK;
}

// a dedupe group from a test hook's arguments (who: the hook's name for the error text)
static int hook_group(DedupeGroup& G, const char* who, const float lamp[3], int32_t count, const uint32_t* seed_prev,
                      const uint32_t* seed_next, int32_t seed_mode, int64_t first_gid, int64_t n)
{
    if (!lamp || !seed_prev || !seed_next || count < 2 || count > DEDUPE_MAX)
        return fail(UVRT_ERR_INVALID, "%s: null argument, or count outside [2,%d]", who, DEDUPE_MAX);
    memset(&G, 0, sizeof G);
    G.lx = lamp[0]; G.ly = lamp[1]; G.lz = lamp[2];
    G.seed_mode = seed_mode;
    G.count = count;
    G.first_gid = first_gid; G.n = n;
    for (int j = 0; j < count; ++j) { G.seed_prev[j] = seed_prev[j]; G.seed_next[j] = seed_next[j]; }
    if (!dedupe_group_ok(G)) return fail(UVRT_ERR_INVALID, "%s: these launches cannot form a dedupe group", who);
    return UVRT_OK;
}
static bool chunk_ok(const DedupeGroup& G, int64_t chunk_first, int64_t chunk_n)
{
    return chunk_n > 0 && chunk_first >= G.first_gid && chunk_first + chunk_n <= G.first_gid + G.n;
}
// a device hook's group as a batch of this group alone plans it: one piece, its classes dealt with the context's class count
// (no byte budget) and its period table through them
static void hook_piece_tables(const uvrt_ctx* c, std::vector<Piece>& one)
{
    Piece& pc = one[0];
    std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
    pc.kc = pc.G.count;
    pc.dd = true;
    if (c->dedupe_classes > 0 && pc.kc <= DEDUPE_CLASS_LAUNCHES)
        pc.ncand = dedupe_class_tally(pc.G, table.data(), pc.cand, c->dedupe_classes, &pc.keys);
    const int first_plane = 0;
    deal_classes(one, c->dedupe_classes, pc.kc, &first_plane);
    if (c->dedupe_periodic) dedupe_periodic_build(pc.G, pc.cls, table.data(), pc.per);
}

}  // namespace uvrt_impl

extern "C" {

int uvrt_trace_batch(uvrt_ctx* c, const float* lamps, float light_length, int32_t count, int64_t first_gid, int64_t n)
{
    uvrt_launch launches[MAX_BATCH];
    memset(launches, 0, sizeof launches);
    if (lamps && count > 0 && count <= MAX_BATCH)
        for (int k = 0; k < count; ++k) {
            memcpy(launches[k].from, &lamps[3 * k], 12);
            launches[k].kind = UVRT_LAUNCH_STOP;
        }
    return trace_launches(c, lamps ? launches : nullptr, light_length, count, first_gid, n, "uvrt_trace_batch");
}

int uvrt_trace_batch_launches(uvrt_ctx* c, const uvrt_launch* launches, float light_length, int32_t count, int64_t first_gid,
                              int64_t n)
{
    return trace_launches(c, launches, light_length, count, first_gid, n, "uvrt_trace_batch_launches");
}

int uvrt_batch_traced_rays(uvrt_ctx* c, int64_t* out)
{
    if (!c || !out) return fail(UVRT_ERR_INVALID, "uvrt_batch_traced_rays: null argument");
    if (c->b_traced_known < 0) return fail(UVRT_ERR_INVALID, "uvrt_batch_traced_rays: no batch has been traced");
    int64_t total = c->b_traced_known;
    if (c->b_traced_chunks > 0) {
        std::vector<uint32_t> counts((size_t)c->b_traced_chunks);
        if (int rc = range_copy(c, c->bs[c->b_set].dd_counts.p, 4, counts.data(), 0, c->b_traced_chunks, hipMemcpyDeviceToHost)) return rc;
        for (uint32_t v : counts) total += v;
    }
    *out = total;
    return UVRT_OK;
}

int uvrt_batch_deposits(uvrt_ctx* c, int64_t* out)
{
    if (!c || !out) return fail(UVRT_ERR_INVALID, "uvrt_batch_deposits: null argument");
    if (c->b_traced_known < 0) return fail(UVRT_ERR_INVALID, "uvrt_batch_deposits: no batch has been traced");
    int64_t total = 0;
    if (c->b_traced_chunks > 0) {      // (the deposit counts follow the ray counts)
        std::vector<uint32_t> counts(2 * (size_t)c->b_traced_chunks);
        if (int rc = range_copy(c, c->bs[c->b_set].dd_counts.p, 4, counts.data(), 0, 2 * c->b_traced_chunks, hipMemcpyDeviceToHost)) return rc;
        for (int32_t i = 0; i < c->b_traced_chunks; ++i) total += counts[(size_t)c->b_traced_chunks + (size_t)i];
    }
    *out = total;
    return UVRT_OK;
}

int uvrt_batch_residue(uvrt_ctx* c, int64_t* nonzero)
{
    if (!c || !nonzero) return fail(UVRT_ERR_INVALID, "uvrt_batch_residue: null argument");
    if (c->b_count > 0) return fail(UVRT_ERR_INVALID, "uvrt_batch_residue: the traced batch has not been replayed (uvrt_replay_batch)");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    HIP_TRY(hipStreamSynchronize(c->stream));
    // the whole allocation of both sets' planes -- launch planes at any R and the class planes behind them -- piece by piece
    // through one host buffer
    const size_t piece = (size_t)16 << 20;      // ints
    std::vector<int32_t> host;
    int64_t total = 0;
    for (const uvrt_ctx::BatchSet& S : c->bs) {
        const size_t ints = S.planes.p ? S.planes.bytes / 4 : 0;
        for (size_t at = 0; at < ints; at += piece) {
            const size_t m = std::min(piece, ints - at);
            host.resize(std::max(host.size(), m));
            if (int rc = copy_sync(c, host.data(), (const int32_t*)S.planes.p + at, m * 4, hipMemcpyDeviceToHost)) return rc;
            for (size_t i = 0; i < m; ++i) total += host[i] != 0;
        }
    }
    *nonzero = total;
    return UVRT_OK;
}

uint32_t uvrt_seed_input(int64_t gid, const float lamp[3], uint32_t seed_prev, uint32_t seed_next, int32_t seed_mode)
{
    return seed_input(gid, lamp[0], lamp[1], lamp[2], seed_prev, seed_next, seed_mode);
}

int uvrt_dedupe_plan(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next, int32_t seed_mode,
                     int64_t first_gid, int64_t n, uint32_t* masks)
{
    DedupeGroup G;
    if (int rc = hook_group(G, "uvrt_dedupe_plan", masks ? lamp : nullptr, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    for (int k = 0; k < count; ++k)
        for (int64_t i = 0; i < n; ++i) masks[(size_t)k * (size_t)n + (size_t)i] = dedupe_mask(G, k, first_gid + i);
    return UVRT_OK;
}

int uvrt_dedupe_plan_strips(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                            int32_t seed_mode, int64_t first_gid, int64_t n, int32_t tile_keys, int32_t strip_tiles,
                            int64_t chunk_first, int64_t chunk_n, uint32_t* masks)
{
    DedupeGroup G;
    if (int rc = hook_group(G, "uvrt_dedupe_plan_tiled", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!masks || tile_keys <= 0 || strip_tiles <= 0 || !chunk_ok(G, chunk_first, chunk_n))
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_plan_tiled: null masks, no tile width, no strip length, or a chunk outside the range");
    std::vector<uint32_t> table((size_t)tile_keys);
    dedupe_plan_tiled(G, tile_keys, strip_tiles, chunk_first, chunk_n, table.data(), masks);
    return UVRT_OK;
}

int uvrt_dedupe_plan_tiled(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                           int32_t seed_mode, int64_t first_gid, int64_t n, int32_t tile_keys, int64_t chunk_first,
                           int64_t chunk_n, uint32_t* masks)
{
    return uvrt_dedupe_plan_strips(lamp, count, seed_prev, seed_next, seed_mode, first_gid, n, tile_keys, DEDUPE_STRIP_TILES, chunk_first,
                                   chunk_n, masks);
}

int32_t uvrt_dedupe_classes_default(void) { return DEDUPE_CLASSES_DEFAULT; }

int uvrt_dedupe_classes(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next, int32_t seed_mode,
                        int64_t first_gid, int64_t n, int32_t max_classes, uint32_t* class_masks, int32_t* class_count,
                        int64_t* deposits)
{
    DedupeGroup G;
    if (int rc = hook_group(G, "uvrt_dedupe_classes", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!class_masks || !class_count || max_classes < 0 || max_classes > DEDUPE_CLASS_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_classes: null output, or a maximum outside [0,%d]", DEDUPE_CLASS_MAX);
    std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
    DedupeTally cand[DEDUPE_CLASS_MAX];
    int nc = 0;
    if (max_classes > 0 && count <= DEDUPE_CLASS_LAUNCHES)
        nc = dedupe_class_tally(G, table.data(), cand, max_classes, nullptr);
    for (int i = 0; i < nc; ++i) class_masks[i] = cand[i].mask;
    *class_count = nc;
    if (deposits) {
        DedupeClasses C;
        dedupe_classes_fill(C, class_masks, nc, (uint32_t)count);
        *deposits = dedupe_class_deposits(G, DEDUPE_TILE_KEYS, C, table.data());
    }
    return UVRT_OK;
}

int uvrt_dedupe_mark_device(uvrt_ctx* c, const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                            int32_t seed_mode, int64_t first_gid, int64_t n, int64_t chunk_first, int64_t chunk_n,
                            uint32_t* masks, uint32_t* block_owner_counts)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_dedupe_mark_device: null context");
    Piece pc = {};      // the group alone: no classes, no period table
    if (int rc = hook_group(pc.G, "uvrt_dedupe_mark_device", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!masks || !block_owner_counts || !chunk_ok(pc.G, chunk_first, chunk_n))
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_mark_device: null output, or a chunk outside the range");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    // lane 0's scratch, on the context's stream (what a chunk without pipelining uses); growing it needs the stream idle
    Lane& L = c->lanes[0];
    const size_t nblocks = (size_t)count * (size_t)((chunk_n + DD_SLOTS - 1) / DD_SLOTS);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = L.dd_tmp.ensure((size_t)count * (size_t)chunk_n * 4, false, c->stream)) return rc;
    if (int rc = L.dd_blocks.ensure((size_t)count * (size_t)((chunk_n + 255) / 256) * 4, true, c->stream)) return rc;
    GenDedupeParams dq;
    fill_dedupe_chunk(c, dq, pc, chunk_first, chunk_n, L, 0.0f);
    launch_dedupe_mark(dq, c->stream);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipMemcpyAsync(masks, dq.tmp, (size_t)count * (size_t)chunk_n * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemcpyAsync(block_owner_counts, dq.block_counts, nblocks * 4, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipMemsetAsync(dq.block_counts, 0, nblocks * 4, c->stream));      // as k_dedupe_write would leave it
    HIP_TRY(hipStreamSynchronize(c->stream));
    return UVRT_OK;
}

int uvrt_dedupe_plan_periodic(const float lamp[3], int32_t count, const uint32_t* seed_prev, const uint32_t* seed_next,
                              int32_t seed_mode, int64_t first_gid, int64_t n, int64_t chunk_first, int64_t chunk_n,
                              uint32_t* masks, uint32_t* block_owner_counts, int64_t* from_table)
{
    DedupeGroup G;
    if (int rc = hook_group(G, "uvrt_dedupe_plan_periodic", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!masks || !block_owner_counts || !from_table || !chunk_ok(G, chunk_first, chunk_n))
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_plan_periodic: null output, or a chunk outside the range");
    std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
    DedupeClasses none = {};
    DedupePeriodic T;
    dedupe_periodic_build(G, none, table.data(), T);
    *from_table = dedupe_plan_periodic(G, T, DEDUPE_MARK_KEYS, DEDUPE_STRIP_TILES, DD_SLOTS, chunk_first, chunk_n, table.data(), masks,
                                       block_owner_counts);
    return UVRT_OK;
}

int uvrt_dedupe_generate_device(uvrt_ctx* c, const float lamp[3], float light_length, int32_t count, const uint32_t* seed_prev,
                                const uint32_t* seed_next, int32_t seed_mode, int64_t first_gid, int64_t n, int64_t chunk_first,
                                int64_t chunk_n, float* rays, uint32_t* words, uint32_t* total, uint32_t* deposits)
{
    if (!c) return fail(UVRT_ERR_INVALID, "uvrt_dedupe_generate_device: null context");
    std::vector<Piece> one(1);
    const Piece& pc = one[0];
    if (int rc = hook_group(one[0].G, "uvrt_dedupe_generate_device", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!rays || !words || !total || !deposits || !chunk_ok(pc.G, chunk_first, chunk_n))
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_generate_device: null output, or a chunk outside the range");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    hook_piece_tables(c, one);
    // lane 0's scratch, on the context's stream; growing it needs the stream idle
    Lane& L = c->lanes[0];
    const size_t slots = (size_t)count * (size_t)chunk_n;
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = L.dd_tmp.ensure(slots * 4, false, c->stream)) return rc;
    if (int rc = L.dd_blocks.ensure((size_t)count * (size_t)((chunk_n + 255) / 256) * 4, true, c->stream)) return rc;
    DevBuf out_rays, out_words, out_counts;
    if (int rc = out_rays.ensure(slots * 16, false, c->stream)) return rc;
    if (int rc = out_words.ensure(slots * 4, false, c->stream)) return rc;
    if (int rc = out_counts.ensure(8, true, c->stream)) return rc;
    GenDedupeParams dq;
    fill_dedupe_chunk(c, dq, pc, chunk_first, chunk_n, L, light_length);
    dq.rays = out_rays.as<float4>();
    dq.masks = out_words.as<uint32_t>();
    dq.total = out_counts.as<uint32_t>();
    dq.deposits = out_counts.as<uint32_t>() + 1;
    launch_generate_dedupe(dq, c->stream);
    HIP_TRY(hipGetLastError());
    uint32_t counts[2] = {0u, 0u};
    HIP_TRY(hipMemcpyAsync(counts, dq.total, 8, hipMemcpyDeviceToHost, c->stream));
    HIP_TRY(hipStreamSynchronize(c->stream));
    if ((size_t)counts[0] > slots) return fail(UVRT_ERR_INVALID, "uvrt_dedupe_generate_device: more rays than occurrences");
    if (counts[0] > 0u) {
        HIP_TRY(hipMemcpyAsync(rays, dq.rays, (size_t)counts[0] * 16, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipMemcpyAsync(words, dq.masks, (size_t)counts[0] * 4, hipMemcpyDeviceToHost, c->stream));
        HIP_TRY(hipStreamSynchronize(c->stream));
    }
    *total = counts[0];
    *deposits = counts[1];
    return UVRT_OK;
}

int uvrt_fold_batch(uvrt_ctx* c)
{
    if (!c || c->b_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_fold_batch: no traced batch");
    if (c->b_is_folded) return UVRT_OK;
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    launch_fold_planes(c->bs[c->b_set].planes.as<int32_t>(), c->bs[c->b_set].folded.as<int32_t>(), c->b_count, c->b_repl, c->T, c->helper_prio, c->stream);
    if (c->b_ncls > 0) {      // a launch's total = its own plane + the class planes of the masks that hold it
        FoldClassParams q;
        memset(&q, 0, sizeof q);
        q.planes = c->bs[c->b_set].planes.as<int32_t>();
        q.folded = c->bs[c->b_set].folded.as<int32_t>();
        q.plane_stride = (int64_t)c->b_repl * c->T;
        q.nplanes = c->b_count;
        q.ncls = c->b_ncls;
        q.cls_replicas = c->b_cls_repl;
        q.T = c->T;
        q.prio = c->helper_prio;
        memcpy(q.launches, c->b_cls_launches, sizeof(uint64_t) * (size_t)c->b_ncls);
        launch_fold_classes(q, c->stream);
    }
    HIP_TRY(hipGetLastError());
    c->b_is_folded = true;
    return UVRT_OK;          // on the context's stream like everything else that touches the set until its replay
}

int uvrt_replay_batch(uvrt_ctx* c, const uvrt_replay_op* ops, int32_t count, int32_t tri_count)
{
    if (!c || !ops || c->b_count <= 0) return fail(UVRT_ERR_INVALID, "uvrt_replay_batch: no traced batch");
    if (count != c->b_count) return fail(UVRT_ERR_INVALID, "uvrt_replay_batch: %d operations for a batch of %d launches", count, c->b_count);
    if (tri_count < 0 || tri_count > c->T) return fail(UVRT_ERR_INVALID, "uvrt_replay_batch: bad tri_count");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    ReplayParams p;
    memset(&p, 0, sizeof p);
    p.photon_map = c->photon_map.as<double>();
    p.max_map = c->max_map.as<double>();
    p.planes = c->bs[c->b_set].planes.as<int32_t>();
    p.folded = c->bs[c->b_set].folded.as<int32_t>();
    p.dosage = c->dosage.as<float>();
    p.color = c->color.as<float>();
    p.area = c->area.as<float>();
    p.plane_stride = (int64_t)c->b_repl * c->T;
    p.replicas = c->b_repl;
    p.T = c->T;
    p.bound = tri_count;
    p.count = count;
    p.is_folded = c->b_is_folded ? 1 : 0;
    p.prio = c->helper_prio;
    p.nplanes = c->b_count;
    p.ncls = c->b_ncls;
    p.cls_replicas = c->b_cls_repl;
    for (int k = 0; k < count; ++k)
        for (int cl = 0; cl < c->b_ncls; ++cl)
            if ((c->b_cls_launches[cl] >> c->b_phys[k]) & 1ull) p.class_of[k] |= 1ull << cl;
    for (int k = 0; k < count; ++k) {
        if (ops[k].which_map != UVRT_MAP_SUM && ops[k].which_map != UVRT_MAP_MAX)
            return fail(UVRT_ERR_INVALID, "uvrt_replay_batch: which_map must be 0 or 1");
        p.ops[k].plane = c->b_phys[k];
        p.ops[k].duration = ops[k].duration;
        p.ops[k].shade = ops[k].shade;
        p.ops[k].which_map = ops[k].which_map;
        p.ops[k].photons_per_light = ops[k].photons_per_light;
        p.ops[k].scaled_power = ops[k].scaled_power;
        p.ops[k].min_value = ops[k].min_value;
        p.ops[k].threshold_view = ops[k].threshold_view;
    }
    launch_replay_batch(p, c->stream);
    HIP_TRY(hipGetLastError());
    if (tri_count < c->T) {     // a partial replay (calibration's 2-triangle scene never does this): clear the rest
        if (c->b_is_folded) HIP_TRY(hipMemsetAsync(c->bs[c->b_set].folded.p, 0, c->bs[c->b_set].folded.bytes, c->stream));
        else HIP_TRY(hipMemsetAsync(c->bs[c->b_set].planes.p, 0, c->bs[c->b_set].planes.bytes, c->stream));
    }
    HIP_TRY(hipEventRecord(c->bs[c->b_set].free_ev, c->stream));    // the set may be traced into again
    c->b_count = 0;
    c->b_is_folded = false;
    // later accumulate / Shade work waits for this replay; the next batch's generate / extend do not
    return mark_map_fence(c);
}

int uvrt_read_batch_counts(uvrt_ctx* c, int32_t launch, int32_t* out, int32_t first, int32_t count)
{
    if (!c || c->b_count <= 0 || launch < 0 || launch >= c->b_count)
        return fail(UVRT_ERR_INVALID, "uvrt_read_batch_counts: no such launch in the traced batch");
    if (int rc = uvrt_fold_batch(c)) return rc;
    if (!range_ok(out, first, count, c->T)) return fail(UVRT_ERR_INVALID, "uvrt_read_batch_counts: bad range");
    return range_copy(c, c->bs[c->b_set].folded.as<int32_t>() + (size_t)c->b_phys[launch] * c->T, 4, out, first, count, hipMemcpyDeviceToHost);
}

}  // extern "C"

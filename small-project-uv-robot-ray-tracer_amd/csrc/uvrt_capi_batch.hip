// uvrt_capi_batch.hip -- batched tracing: several launches in one go, one count plane per launch
// (the C ABI of include/uvrt.h over the HIP kernels; the context and its helpers are in uvrt_ctx.h)
#include "uvrt_ctx.h"

using namespace uvrt;
using namespace uvrt_impl;

namespace uvrt_impl {

// The chunk's key tiles and the strip of them a wave of the mark pass walks: DEDUPE_STRIP_TILES, and up to twice that where
// the chunk still keeps 4 096 waves busy -- a longer strip spreads its one search over more tiles, a shorter one leaves a
// small chunk more waves to cover each other's waits (DESIGN.md section 15 has the sweep).
static void mark_tiles(const uvrt_ctx* c, GenDedupeParams& q)
{
    dedupe_tile_range(q.g, q.g0, q.gn, DEDUPE_MARK_KEYS, q.key_lo, q.tiles);
    // ... of the key intervals that the group's period table (q.per; count 0: none) leaves to the mark pass: the tiles it
    // walks (strips of one), then the strips
    q.gaps = dedupe_periodic_gaps(q.per, q.key_lo, q.tiles * DEDUPE_MARK_KEYS, DEDUPE_MARK_KEYS, 1, q.gap_key, q.gap_keys, q.gap_strip0);
    const int64_t walked = q.gap_strip0[q.gaps];
    // (with a table few tiles are left and a wave's walk is all the pass takes: strips down to one tile)
    const int64_t fit = std::min<int64_t>(2 * DEDUPE_STRIP_TILES, std::max<int64_t>(q.per.count > 0 ? 1 : DEDUPE_STRIP_TILES, walked / 4096));
    q.strip_tiles = c->dedupe_strip > 0 ? c->dedupe_strip : (int32_t)fit;
    q.gaps = dedupe_periodic_gaps(q.per, q.key_lo, q.tiles * DEDUPE_MARK_KEYS, DEDUPE_MARK_KEYS, q.strip_tiles, q.gap_key, q.gap_keys, q.gap_strip0);
}

// uvrt_trace_batch and uvrt_trace_batch_launches (`who` names the caller in the error texts): generate + extend for `count`
// launches, stops grouped by lamp column and traced by k_extend6, sweeps as one further group traced by the plane-aware
// k_extend_free.  Physical planes: the stops' groups first, then the sweeps in logical order.
static int trace_launches(uvrt_ctx* c, const uvrt_launch* launches, float light_length, int32_t count, int64_t first_gid,
                          int64_t n, const char* who)
{
    if (!c || !launches || !c->have_scene) return fail(UVRT_ERR_INVALID, "%s: null argument or no scene", who);
    if (count <= 0 || count > MAX_BATCH) return fail(UVRT_ERR_INVALID, "%s: count must be in [1,%d]", who, MAX_BATCH);
    if (n <= 0 || first_gid < 0 || first_gid + n > (int64_t)INT32_MAX)
        return fail(UVRT_ERR_INVALID, "%s: bad global-id range", who);
    if (c->b_count > 0) return fail(UVRT_ERR_INVALID, "%s: the previous batch has not been replayed (uvrt_replay_batch)", who);
    if (c->record_hits || c->sort_bits != 0)
        return fail(UVRT_ERR_INVALID, "%s: per-ray hit records and ray ordering are per-launch features", who);
    int nsweeps = 0;
    for (int k = 0; k < count; ++k) {
        if (launches[k].kind != UVRT_LAUNCH_STOP && launches[k].kind != UVRT_LAUNCH_SWEEP)
            return fail(UVRT_ERR_INVALID, "%s: launch %d: kind must be UVRT_LAUNCH_STOP or UVRT_LAUNCH_SWEEP", who, k);
        nsweeps += launches[k].kind == UVRT_LAUNCH_SWEEP;
    }
    if (nsweeps > 0 && c->seed_mode != 0)
        return fail(UVRT_ERR_INVALID, "%s: seed mode 1 models the SEED race of generate.cl only; a sweep needs "
                    "uvrt_set_seed_mode(ctx, 0)", who);
    if (nsweeps > 0 && c->flavour != 0 && c->flavour != 1)
        return fail(UVRT_ERR_INVALID, "%s: rays with origins of their own are traced in flavours 0 and 1 only "
                    "(uvrt_set_flavour %d)", who, c->flavour);
    const int nstops = count - nsweeps;
    if (int rc = set_device(c)) return rc;
    const int64_t n_pad = (n + 63) / 64 * 64;
    // deposit replicas per plane: the contention on a hot triangle's counter grows with the rays per plane
    // (16 replicas for 2 M rays), and every replica is read and zeroed again by the replay -- a shard of a launch
    // gets by with 8 (one per XCD)
    // (a fused batch is happiest with 8-12 replicas even at 2 M rays per plane: +0.4 % over 16, profiles/r03/r03_knobs_room.txt;
    // the per-launch path keeps the context's 16)
    int R = std::min(c->replicas, 12);
    if ((int64_t)R * 131072 > 2 * n) R = std::min(c->replicas, 8);
    if ((uint64_t)count * (uint64_t)n_pad >= ((uint64_t)1 << 30) || (uint64_t)count * (uint64_t)R * (uint64_t)c->T >= ((uint64_t)1 << 32))
        return fail(UVRT_ERR_INVALID, "%s: %d launches x %lld rays exceed one batch (2^30 ray slots, 2^32 counters)", who, count, (long long)n);

    // group the stops by lamp column (x, z): the per-launch node-pair records depend on it only
    int group_of[MAX_BATCH], ngroups = 0, gfirst[MAX_BATCH], gsize[MAX_BATCH] = {};
    float gx[MAX_BATCH], gz[MAX_BATCH];
    for (int k = 0; k < count; ++k) {
        if (launches[k].kind != UVRT_LAUNCH_STOP) continue;
        const float* lamp = launches[k].from;
        int g = 0;
        for (; g < ngroups; ++g)
            if (memcmp(&gx[g], &lamp[0], 4) == 0 && memcmp(&gz[g], &lamp[2], 4) == 0) break;
        if (g == ngroups) { gx[g] = lamp[0]; gz[g] = lamp[2]; ++ngroups; }
        group_of[k] = g;
        ++gsize[g];
    }
    for (int g = 0, acc = 0; g < ngroups; ++g) { gfirst[g] = acc; acc += gsize[g]; }
    GenBatchParams gp;                  // the stops, by physical plane
    memset(&gp, 0, sizeof gp);
    SweepBatchParams sp;                // the sweeps, by physical plane - nstops
    memset(&sp, 0, sizeof sp);
    int32_t phys[MAX_BATCH];            // committed (c->b_phys) with the batch
    uint32_t seed_after = c->seed;
    {
        int fill[MAX_BATCH] = {}, sfill = 0;
        uint32_t seed = c->seed;
        for (int k = 0; k < count; ++k) {                    // logical order: the SEED chain
            const uvrt_launch& l = launches[k];
            if (l.kind == UVRT_LAUNCH_STOP) {
                const int g = group_of[k], ph = gfirst[g] + fill[g]++;
                phys[k] = ph;
                gp.lx[ph] = l.from[0]; gp.ly[ph] = l.from[1]; gp.lz[ph] = l.from[2];
                gp.seed_prev[ph] = seed;
                seed = uvrt_seed_next_mode(l.from, light_length, seed, c->seed_mode);
                gp.seed_next[ph] = seed;
            } else {
                const int j = sfill++;
                phys[k] = nstops + j;
                sp.fx[j] = l.from[0]; sp.fy[j] = l.from[1]; sp.fz[j] = l.from[2];
                sp.tx[j] = l.to[0]; sp.ty[j] = l.to[1]; sp.tz[j] = l.to[2];
                sp.seed_prev[j] = seed;
                seed = uvrt_seed_next_sweep(l.from, light_length, seed);
                sp.seed_next[j] = seed;
            }
        }
        seed_after = seed;              // committed with the batch: a failed call leaves the SEED chain where it was
    }
    // The columns in PIECES: a dedupe group each (uvrt_dedupe.h: 2..31 launches of one bit-identical lamp, every distinct ray
    // traced once), or launches traced as they are -- a column of one, lamps that differ in y, a range or a lamp outside
    // dedupe_group_ok, uvrt_set_dedupe(0), a kernel variant other than the default's code (the deduped kernel exists for leaf
    // period 2 with the LDS cache only), the developer build's skip-generate probe.  A longer column is split evenly (33
    // launches: 17 + 16).
    struct Piece {
        int g, k0, kc; bool dd; int64_t chunk_gids; DedupeGroup G;
        DedupeTally cand[DEDUPE_CLASS_MAX]; int ncand; double keys;       // its owners' multi-bit masks by sampled frequency
        int ncls, cls_base; DedupeClasses cls;                            // the classes it gets, from class plane cls_base on
        DedupePeriodic per;                                               // its period table (count 0: none)
    };
    std::vector<Piece> pieces;
    size_t dd_chunks = 0, dd_tmp_bytes = 0, dd_block_bytes = 0;
    bool may_dedupe = c->dedupe && variant_code6(c->variant) == 1;
#ifdef UVRT_DEV_VARIANTS
    may_dedupe = may_dedupe && c->probe_skip_generate <= 0;
#endif
    for (int g = 0; g < ngroups; ++g) {
        bool same_lamp = may_dedupe && gsize[g] >= 2;
        for (int j = 1; same_lamp && j < gsize[g]; ++j) same_lamp = memcmp(&gp.ly[gfirst[g]], &gp.ly[gfirst[g] + j], 4) == 0;
        const int npieces = same_lamp ? (gsize[g] + DEDUPE_MAX - 1) / DEDUPE_MAX : 1;
        const int per_piece = (gsize[g] + npieces - 1) / npieces;
        for (int k0 = 0; k0 < gsize[g]; k0 += per_piece) {
            Piece pc;
            memset(&pc, 0, sizeof pc);
            pc.g = g; pc.k0 = k0; pc.kc = std::min(per_piece, gsize[g] - k0);
            const int ph0 = gfirst[g] + k0;
            if (same_lamp && pc.kc >= 2) {
                DedupeGroup& G = pc.G;
                G.lx = gp.lx[ph0]; G.ly = gp.ly[ph0]; G.lz = gp.lz[ph0];
                G.seed_mode = c->seed_mode;
                G.count = pc.kc;
                G.first_gid = first_gid; G.n = n;
                for (int j = 0; j < pc.kc; ++j) { G.seed_prev[j] = gp.seed_prev[ph0 + j]; G.seed_next[j] = gp.seed_next[ph0 + j]; }
                pc.dd = dedupe_group_ok(G);
            }
            if (pc.dd) {
                // a chunk: a gid range across all the piece's launches, sized by its upper bound (no duplicates)
                pc.chunk_gids = std::max<int64_t>(64, (int64_t)(c->dedupe_chunk_bytes / ((size_t)pc.kc * 16)) / 64 * 64);
                // ... and the range dealt evenly over that many chunks (a short last chunk leaves one lane idle at the end)
                const int64_t nch = (n + pc.chunk_gids - 1) / pc.chunk_gids;
                pc.chunk_gids = ((n + nch - 1) / nch + 63) / 64 * 64;
                const int64_t gn = std::min(pc.chunk_gids, n);
                dd_chunks += (size_t)((n + pc.chunk_gids - 1) / pc.chunk_gids);
                dd_tmp_bytes = std::max(dd_tmp_bytes, (size_t)pc.kc * (size_t)gn * 4);
                dd_block_bytes = std::max(dd_block_bytes, (size_t)pc.kc * (size_t)((gn + 255) / 256) * 4);
            }
            pieces.push_back(pc);
        }
    }
    // The batch goes into the buffer set the previous batch did NOT use: its lanes start at once -- in the drain of
    // the previous batch, while that one is still being folded / reduced / replayed on the context's stream -- and
    // only wait for the set's last replay (free_ev), which is two batches back.  Anything that has to touch memory
    // the lanes may still read (growing a buffer, new per-launch records) first waits for everything.
    const int set = c->b_set ^ 1;
    uvrt_ctx::BatchSet& S = c->bs[set];
    int rc;
    const size_t plane_ints = (size_t)R * (size_t)c->T;
    // full planes are allocated for the context's replica count: R only shrinks the part of it that is used
    const size_t plane_alloc = (size_t)c->replicas * (size_t)c->T;
    // The mask classes of the dedupe groups (uvrt_dedupe.h "mask classes"): every group's candidates from a sample of its key
    // tiles -- a function of the group alone, found here on the host with no word from the device -- and the class planes of
    // the set dealt to the groups by sampled frequency, most frequent first.  The planes sit behind the launch planes, at
    // most class_cap of them: the set's byte budget, one bit each in ReplayParams::class_of, every offset below 2^32.
    const bool classes_on = c->dedupe_classes > 0 && dd_chunks > 0;
    int class_cap = 0, total_cls = 0;
    const int cls_repl = std::max(1, std::min(c->dedupe_class_replicas, R));
    if (classes_on) {
        const uint64_t room = (((uint64_t)1 << 32) - 1) / (uint64_t)plane_ints;
        class_cap = (int)std::min<uint64_t>({(uint64_t)MAX_CLASS_PLANES, (uint64_t)(c->dedupe_class_bytes / (plane_ints * 4)),
                                             room > (uint64_t)count ? room - (uint64_t)count : 0});
        std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
        for (Piece& pc : pieces)
            if (pc.dd && pc.kc <= DEDUPE_CLASS_LAUNCHES)
                pc.ncand = dedupe_class_tally(pc.G, table.data(), pc.cand, c->dedupe_classes, &pc.keys);
        while (total_cls < class_cap) {
            Piece* best = nullptr;
            double best_f = 0.0;
            for (Piece& pc : pieces) {
                if (pc.ncls >= pc.ncand) continue;
                const double f = pc.cand[pc.ncls].n / pc.keys;
                if (f > best_f) { best_f = f; best = &pc; }
            }
            if (!best) break;
            ++best->ncls;
            ++total_cls;
        }
        int base = 0;
        for (Piece& pc : pieces) {
            uint32_t masks[DEDUPE_CLASS_MAX];
            for (int i = 0; i < pc.ncls; ++i) masks[i] = pc.cand[i].mask;
            pc.cls_base = base;
            // (a class plane's index counts from the group's first launch plane, as a launch's does)
            dedupe_classes_fill(pc.cls, masks, pc.ncls, (uint32_t)(count - (gfirst[pc.g] + pc.k0) + base));
            base += pc.ncls;
        }
    }
    // The period tables of the dedupe groups (uvrt_dedupe.h "period table"), words through the classes just dealt: a function
    // of the group alone, built here at every call with no word from the device; they travel in the kernels' arguments.
    if (c->dedupe_periodic && dd_chunks > 0) {
        std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
        for (Piece& pc : pieces)
            if (pc.dd) dedupe_periodic_build(pc.G, pc.cls, table.data(), pc.per);
    }
    const size_t planes_bytes = (size_t)count * plane_alloc * 4 + (size_t)class_cap * plane_ints * 4;
    // growing a buffer needs the device idle (hipFree / hipMalloc); new per-launch records only need the context's stream
    // ordered after the lanes' earlier work -- no host synchronisation, so a new lamp position costs its kernels only
    bool dd_scratch_short = false;      // (every lane a chunk may run on: 0 without pipelining, else 1..batch_lanes)
    for (int l = 0; l <= c->batch_lanes; ++l)
        dd_scratch_short = dd_scratch_short || c->lanes[l].dd_tmp.bytes < dd_tmp_bytes || c->lanes[l].dd_blocks.bytes < dd_block_bytes;
    const bool need_alloc = S.rays.bytes < (size_t)count * (size_t)n_pad * 16 || S.planes.bytes < planes_bytes ||
                            S.folded.bytes < (size_t)count * (size_t)c->T * 4 || (int)c->b_recs.size() < ngroups || !S.free_ev ||
                            S.oxz.bytes < (size_t)nsweeps * (size_t)n_pad * 8 || (nsweeps > 0 && !c->free_recs_valid) ||
                            (dd_chunks > 0 && (S.masks.bytes < (size_t)count * (size_t)n_pad * 4 || S.dd_counts.bytes < dd_chunks * 8 ||
                                               dd_scratch_short));
    bool recs_stale = false;
    const uint32_t* gperm[MAX_BATCH] = {};
    uint64_t ggen[MAX_BATCH] = {};
    uvrt_ctx::HotEntry* fresh[MAX_BATCH];               // lamps the context has not seen: their set-ups go in ONE launch
    uint32_t fresh_prev[MAX_BATCH], fresh_next[MAX_BATCH];
    int nfresh = 0;
    for (int g = 0; g < ngroups; ++g) {
        gperm[g] = c->have_perm ? c->perm.as<uint32_t>() : nullptr;
        bool is_fresh = false;
        if (!gperm[g] && (int64_t)gsize[g] * n >= 16384) {
            const int ph = gfirst[g];      // the group's first launch lends its lamp and seeds to the statistics
            const float gl[3] = {gp.lx[ph], gp.ly[ph], gp.lz[ph]};
            uvrt_ctx::HotEntry* e = nullptr;
            if (int rcp = hot_lookup(c, gl, c->stream, &gperm[g], &e)) return rcp;
            if (e) {
                gperm[g] = e->perm;
                fresh[nfresh] = e; fresh_prev[nfresh] = gp.seed_prev[ph]; fresh_next[nfresh] = gp.seed_next[ph];
                ++nfresh;
                is_fresh = true;
            }
        }
        ggen[g] = perm_generation(c, gperm[g]);
        if (g >= (int)c->b_recs_key.size() || !c->b_recs_key[g].holds(gx[g], gz[g], gperm[g], ggen[g]) || is_fresh) {
            recs_stale = true;
            if (g < (int)c->b_recs_key.size()) c->b_recs_key[g].tag.valid = false;
        }
    }
    if (nfresh > 0)
        if (int rcb = hot_build(c, fresh, fresh_prev, fresh_next, nfresh, light_length, c->stream, 0)) return rcb;
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
        if ((rc = S.oxz.ensure((size_t)nsweeps * (size_t)n_pad * 8, false, c->stream))) return rc;      // (8 B of origin per photon of a sweep)
        if (grown) HIP_TRY(hipEventRecord(S.free_ev, c->stream));      // the zero fill is the set's "last replay"
        while ((int)c->b_recs.size() < ngroups) {
            DevBuf b;
            if ((rc = b.ensure(((size_t)c->npairs + (size_t)c->T + 1) * 64, true, c->stream))) return rc;
            launch_prepare_leaves6(c->ltris.as<LeafTri>(), b.p, c->npairs, c->T, c->stream);
            c->b_recs.push_back(std::move(b));
        }
        c->b_recs_key.resize(c->b_recs.size());
        for (int l = 1; l <= c->batch_lanes; ++l)
            if ((rc = c->lanes[l].ovf.ensure(side_ovf_bytes(c), false, c->stream))) return rc;
        if (dd_chunks > 0) {      // the deduped chunks' masks and counts, and every lane's scratch between the generate passes
            if ((rc = S.masks.ensure((size_t)count * (size_t)n_pad * 4, false, c->stream))) return rc;
            // (not zeroed: a chunk's generate runs on its lane BEFORE the lane waits for this stream, and writes its count;
            //  the chunks' ray counts first, their deposit counts behind them)
            if ((rc = S.dd_counts.ensure(dd_chunks * 8, false, c->stream))) return rc;
            // (dd_blocks zeroed: k_dedupe_mark adds its owners to it and k_dedupe_write leaves it zero again.  A chunk's generate
            //  does not wait for this stream, so the zero fill is waited for here, where a buffer has grown)
            for (int l = 0; l <= c->batch_lanes; ++l) {
                if ((rc = c->lanes[l].dd_tmp.ensure(dd_tmp_bytes, false, c->stream))) return rc;
                if ((rc = c->lanes[l].dd_blocks.ensure(dd_block_bytes, true, c->stream))) return rc;
            }
            HIP_TRY(hipStreamSynchronize(c->stream));
        }
    }
    if (need_alloc || recs_stale) {
        // per-launch records of the lamp columns whose array holds something else
        for (int g = 0; g < ngroups; ++g) {
            uvrt_ctx::RecsKey& key = c->b_recs_key[g];
            if (key.holds(gx[g], gz[g], gperm[g], ggen[g])) continue;
            launch_prepare_launch6(c->pairs.as<PairRec>(), c->b_recs[g].p, gx[g], gz[g], c->npairs, gperm[g], c->helper_prio, c->stream);
            key = {{true, gx[g], gz[g]}, gperm[g], ggen[g]};
        }
        // the scene's free records, on first use (the lanes are joined above, the fence below covers them)
        if (nsweeps > 0 && !c->free_recs_valid)
            if ((rc = make_free_records(c))) return rc;
        HIP_TRY(hipGetLastError());
        if (int rcf = mark_fence(c)) return rcf;         // the lanes' next work waits for the records
    }
    // Launches in CHUNKS of a few planes: generate + fused extend of a chunk on one launch lane, chunks alternating
    // over the lanes.  A chunk's rays (16 B each) are sized to stay in the Infinity Cache between the generate
    // that writes them and the extend that reads them (a refill that has to go to HBM stalls its wave for
    // microseconds), and the next chunk's generate and first waves run in the drain of the previous one.
    bool lane_waited[uvrt_ctx::MAXL] = {};
    // (a plane's offset shares its register with the exact-step flag, PLANE_OFF6: a chunk's planes stay below 2^31 counters)
    const size_t planes_31 = std::max<size_t>(1, (((size_t)1 << 31) - 1) / plane_ints);
    const int per_chunk = (int)std::min(planes_31, std::max<size_t>(1, c->batch_chunk_bytes / ((size_t)n_pad * 16)));
    // every error return below leaves the launch-lane rotation as it found it
    struct LaneGuard {
        uvrt_ctx* c; int lane; uint64_t chunks; bool armed;
        ~LaneGuard() { if (armed) { c->lane = lane; c->b_chunks = chunks; } }
    } guard{c, c->lane, c->b_chunks, true};
    // The lane of the next chunk.  Two SIDE lanes in turn: the context's own stream carries the fold / reduce / replay of the
    // previous batch, which a chunk enqueued there would have to wait for.  The chunk's rays depend on nothing but their
    // buffer: generate goes to the lane's stream (*ls) BEFORE the lane waits for the context's stream (lane_stream: new
    // records, a hot-record set-up), so it runs beside them.
    auto next_chunk_lane = [&](hipStream_t* ls) -> int {
        c->lane = c->pipeline ? 1 + (int)(c->b_chunks++ % (uint64_t)c->batch_lanes) : 0;
        *ls = stream_of(c, c->lane);
        if (c->lane != 0) cur_lane(c).used = true;
        if (!lane_waited[c->lane]) {      // the set's previous occupant has been replayed (two batches back)
            HIP_TRY(hipStreamWaitEvent(*ls, S.free_ev, 0));
            lane_waited[c->lane] = true;
        }
        return UVRT_OK;
    };
    // what the fused extend of a chunk of kc planes from physical plane ph0 on gets besides its rays and records
    auto set_planes = [&](ExtendParams& p, int ph0, int kc) {
        p.counts = S.planes.as<int32_t>() + (size_t)ph0 * plane_ints;
        p.count_replicas = R;
        p.count_stride = c->T;
        p.n = (int64_t)kc * n_pad;
        p.plane_batches = (uint32_t)(n_pad / 64);
        p.plane_n = (uint32_t)n;
        p.plane_stride = (uint32_t)plane_ints;
    };
    const int per_cu = variant_per_cu(c->variant, c->pipeline ? 7 : 8);
    int64_t traced = 0;                  // rays handed to k_extend6 with their count known here; the deduped chunks' counts stay on the device
    size_t dd_used = 0;
    for (const Piece& pc : pieces) {
        const int g = pc.g;
        if (pc.dd) {
            // a dedupe group: chunks are gid ranges across all its launches; whether an occurrence is an owner is decided over
            // the whole call's range, a chunk only says where the owner's ray is generated
            for (int64_t g0 = 0; g0 < n; g0 += pc.chunk_gids) {
                const int64_t gn = std::min(pc.chunk_gids, n - g0);
                const int ph0 = gfirst[g] + pc.k0;
                hipStream_t ls;
                if (int rcl = next_chunk_lane(&ls)) return rcl;
                const size_t at = (size_t)ph0 * (size_t)n_pad + (size_t)pc.kc * (size_t)g0;
                GenDedupeParams dq;
                memset(&dq, 0, sizeof dq);
                dq.g = pc.G;
                dq.rays = S.rays.as<float4>() + at;
                dq.masks = S.masks.as<uint32_t>() + at;
                dq.total = S.dd_counts.as<uint32_t>() + dd_used;
                dq.deposits = S.dd_counts.as<uint32_t>() + dd_chunks + dd_used++;
                dq.cls = pc.cls;
                dq.per = pc.per;
                dq.tmp = cur_lane(c).dd_tmp.as<uint32_t>();
                dq.g0 = first_gid + g0;
                dq.gn = gn;
                dq.block_counts = cur_lane(c).dd_blocks.as<uint32_t>();
                mark_tiles(c, dq);
                dq.light_length = light_length;
                dq.prio = c->helper_prio;
                launch_generate_dedupe(dq, ls);
                if (int rcl = lane_stream(c, &ls)) return rcl;      // extend: after the fence
                ExtendParams p;
                fill_launch(c, p, gx[g], gz[g]);
                p.rays = dq.rays;
                p.masks = dq.masks;
                p.n_dev = dq.total;
                p.counts = S.planes.as<int32_t>() + (size_t)ph0 * plane_ints;
                p.count_replicas = R;
                p.count_stride = c->T;
                p.n = (int64_t)pc.kc * gn;
                p.plane_stride = (uint32_t)plane_ints;
                p.cls_replicas = pc.cls.count > 0 ? cls_repl : 0;      // (0: the chunk's words are its masks)
                p.recs = c->b_recs[g].p;
                p.perm = gperm[g];
                p.recs_prepared = 1;
                if (int rct = timed_launch(c, ls, who, "the stops' launch", [&] { return launch_extend6_dedupe(p, variant_code6(c->variant), per_cu, ls); }))
                    return rct;
            }
            continue;
        }
        for (int k0 = pc.k0; k0 < pc.k0 + pc.kc; k0 += per_chunk) {
            const int kc = std::min(per_chunk, pc.k0 + pc.kc - k0), ph0 = gfirst[g] + k0;
            traced += (int64_t)kc * n;
            hipStream_t ls;
            if (int rcl = next_chunk_lane(&ls)) return rcl;
            GenBatchParams gq;
            memset(&gq, 0, sizeof gq);
            gq.rays = S.rays.as<float4>() + (size_t)ph0 * (size_t)n_pad;
            gq.n_pad = n_pad;
            gq.first_gid = first_gid;
            gq.n = n;
            gq.light_length = light_length;
            gq.seed_mode = c->seed_mode;
            gq.count = kc;
            gq.prio = c->helper_prio;
            for (int j = 0; j < kc; ++j) {
                gq.lx[j] = gp.lx[ph0 + j]; gq.ly[j] = gp.ly[ph0 + j]; gq.lz[j] = gp.lz[ph0 + j];
                gq.seed_prev[j] = gp.seed_prev[ph0 + j]; gq.seed_next[j] = gp.seed_next[ph0 + j];
            }
#ifdef UVRT_DEV_VARIANTS
            if (!(c->probe_skip_generate > 0 && c->probe_batches >= c->probe_skip_generate))
#endif
            launch_generate_batch(gq, ls);
            if (int rcl = lane_stream(c, &ls)) return rcl;      // extend: after the fence
            ExtendParams p;
            fill_launch(c, p, gx[g], gz[g]);
            p.rays = gq.rays;
            set_planes(p, ph0, kc);
            p.recs = c->b_recs[g].p;
            p.perm = gperm[g];
            p.recs_prepared = 1;
            if (int rct = timed_launch(c, ls, who, "the stops' launch", [&] { return launch_extend6(p, variant_code6(c->variant), per_cu, c->helper_prio, ls); }))
                return rct;
        }
    }
    // The sweeps: one further group (the free records are the scene's, whatever the segment), in chunks of as many bytes --
    // 16 B of ray plus 8 B of origin per photon -- over the same lanes in the same rotation.
    const int per_sweep_chunk = (int)std::min(planes_31, std::max<size_t>(1, c->batch_chunk_bytes / ((size_t)n_pad * 24)));
    for (int k0 = 0; k0 < nsweeps; k0 += per_sweep_chunk) {
        const int kc = std::min(per_sweep_chunk, nsweeps - k0), ph0 = nstops + k0;
        hipStream_t ls;
        if (int rcl = next_chunk_lane(&ls)) return rcl;
        SweepBatchParams sq;
        memset(&sq, 0, sizeof sq);
        sq.rays = S.rays.as<float4>() + (size_t)ph0 * (size_t)n_pad;
        sq.oxz = S.oxz.as<float2>() + (size_t)k0 * (size_t)n_pad;
        sq.n_pad = n_pad;
        sq.first_gid = first_gid;
        sq.n = n;
        sq.light_length = light_length;
        sq.count = kc;
        sq.prio = c->helper_prio;
        for (int j = 0; j < kc; ++j) {
            sq.fx[j] = sp.fx[k0 + j]; sq.fy[j] = sp.fy[k0 + j]; sq.fz[j] = sp.fz[k0 + j];
            sq.tx[j] = sp.tx[k0 + j]; sq.ty[j] = sp.ty[k0 + j]; sq.tz[j] = sp.tz[k0 + j];
            sq.seed_prev[j] = sp.seed_prev[k0 + j]; sq.seed_next[j] = sp.seed_next[k0 + j];
        }
#ifdef UVRT_DEV_VARIANTS
        if (!(c->probe_skip_generate > 0 && c->probe_batches >= c->probe_skip_generate))
#endif
        launch_generate_sweep_batch(sq, ls);
        if (int rcl = lane_stream(c, &ls)) return rcl;      // extend: after the fence
        FreeParams fp;
        fill_launch(c, fp.e, 0.0f, 0.0f);       // (force_exact: the scene's and the variant's conditions; the origins are per ray)
        fp.e.rays = sq.rays;
        fp.oxz = sq.oxz;
        set_planes(fp.e, ph0, kc);
        fp.e.recs = c->free_recs.p;
        if (int rct = timed_launch(c, ls, who, "the free-ray launch", [&] { return launch_extend_free_planes(fp, per_cu, ls); }))
            return rct;
    }
#ifdef UVRT_DEV_VARIANTS
    ++c->probe_batches;
#endif
    guard.armed = false;
    c->seed = seed_after;
    c->lane = 0;
    c->cur_pipelined = false;
    c->last = {};                        // the per-launch generate/extend pairing starts afresh
    c->b_set = set;
    c->b_repl = R;
    c->b_count = count;
    c->b_n = n;
    c->b_npad = n_pad;
    c->b_is_folded = false;
    c->b_traced_known = traced;
    c->b_traced_chunks = (int32_t)dd_used;
    c->b_ncls = total_cls;
    c->b_cls_repl = cls_repl;
    for (const Piece& pc : pieces)
        for (int i = 0; i < pc.ncls; ++i) c->b_cls_launches[pc.cls_base + i] = (uint64_t)pc.cls.mask[i] << (gfirst[pc.g] + pc.k0);
    memcpy(c->b_phys, phys, sizeof(int32_t) * (size_t)count);
    return UVRT_OK;
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
    if (!lamp || !seed_prev || !seed_next || !masks || count < 2 || count > DEDUPE_MAX)
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_plan: null argument, or count outside [2,%d]", DEDUPE_MAX);
    DedupeGroup G;
    memset(&G, 0, sizeof G);
    G.lx = lamp[0]; G.ly = lamp[1]; G.lz = lamp[2];
    G.seed_mode = seed_mode;
    G.count = count;
    G.first_gid = first_gid; G.n = n;
    for (int j = 0; j < count; ++j) { G.seed_prev[j] = seed_prev[j]; G.seed_next[j] = seed_next[j]; }
    if (!dedupe_group_ok(G)) return fail(UVRT_ERR_INVALID, "uvrt_dedupe_plan: these launches cannot form a dedupe group");
    for (int k = 0; k < count; ++k)
        for (int64_t i = 0; i < n; ++i) masks[(size_t)k * (size_t)n + (size_t)i] = dedupe_mask(G, k, first_gid + i);
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
    GenDedupeParams dq;
    memset(&dq, 0, sizeof dq);
    if (int rc = hook_group(dq.g, "uvrt_dedupe_mark_device", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!masks || !block_owner_counts || !chunk_ok(dq.g, chunk_first, chunk_n))
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_mark_device: null output, or a chunk outside the range");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    // lane 0's scratch, on the context's stream (what a chunk without pipelining uses); growing it needs the stream idle
    Lane& L = c->lanes[0];
    const size_t nblocks = (size_t)count * (size_t)((chunk_n + DD_SLOTS - 1) / DD_SLOTS);
    HIP_TRY(hipStreamSynchronize(c->stream));
    if (int rc = L.dd_tmp.ensure((size_t)count * (size_t)chunk_n * 4, false, c->stream)) return rc;
    if (int rc = L.dd_blocks.ensure((size_t)count * (size_t)((chunk_n + 255) / 256) * 4, true, c->stream)) return rc;
    dq.tmp = L.dd_tmp.as<uint32_t>();
    dq.g0 = chunk_first;
    dq.gn = chunk_n;
    dq.block_counts = L.dd_blocks.as<uint32_t>();
    mark_tiles(c, dq);
    dq.prio = c->helper_prio;
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
    GenDedupeParams dq;
    memset(&dq, 0, sizeof dq);
    if (int rc = hook_group(dq.g, "uvrt_dedupe_generate_device", lamp, count, seed_prev, seed_next, seed_mode, first_gid, n)) return rc;
    if (!rays || !words || !total || !deposits || !chunk_ok(dq.g, chunk_first, chunk_n))
        return fail(UVRT_ERR_INVALID, "uvrt_dedupe_generate_device: null output, or a chunk outside the range");
    if (int rc = set_device(c)) return rc;
    if (int rc = join_all(c)) return rc;
    // the group's classes as a batch of this group alone deals them, then its period table
    std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
    if (c->dedupe_classes > 0 && count <= DEDUPE_CLASS_LAUNCHES) {
        DedupeTally cand[DEDUPE_CLASS_MAX];
        uint32_t class_masks[DEDUPE_CLASS_MAX];
        const int nc = dedupe_class_tally(dq.g, table.data(), cand, c->dedupe_classes, nullptr);
        for (int i = 0; i < nc; ++i) class_masks[i] = cand[i].mask;
        dedupe_classes_fill(dq.cls, class_masks, nc, (uint32_t)count);
    }
    if (c->dedupe_periodic) dedupe_periodic_build(dq.g, dq.cls, table.data(), dq.per);
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
    dq.rays = out_rays.as<float4>();
    dq.masks = out_words.as<uint32_t>();
    dq.total = out_counts.as<uint32_t>();
    dq.deposits = out_counts.as<uint32_t>() + 1;
    dq.tmp = L.dd_tmp.as<uint32_t>();
    dq.g0 = chunk_first;
    dq.gn = chunk_n;
    dq.block_counts = L.dd_blocks.as<uint32_t>();
    mark_tiles(c, dq);
    dq.light_length = light_length;
    dq.prio = c->helper_prio;
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

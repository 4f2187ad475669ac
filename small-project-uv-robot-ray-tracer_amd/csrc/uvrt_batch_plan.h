// uvrt_batch_plan.h -- what a batch will enqueue, worked out on the host before anything touches the GPU: the lamp columns and
// physical planes, the SEED chain, the pieces and their chunks, the mask classes and period tables of the dedupe groups, the
// replica count and the scratch sizes.  A function of uvrt_trace_batch_launches' arguments and a dozen context knobs
// (BatchKnobs): no HIP, so tests/tools/batch_plan_check.cpp runs it alone.  uvrt_capi_batch.hip provisions and enqueues from
// the plan; the SEED chain goes through include/uvrt.h's declarations, which the library defines.
#pragma once
#include "../../include/uvrt.h"
#include "uvrt_dedupe.h"

#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <vector>

namespace uvrt {

// what the plan reads from the context
struct BatchKnobs {
    uint32_t seed;                      // SEED before the batch
    int32_t seed_mode;
    int32_t T, replicas;                // the scene's triangles; the context's deposit replicas
    bool may_dedupe;                    // uvrt_set_dedupe, the default kernel variant, no skip-generate probe
    int32_t dedupe_classes, dedupe_class_replicas;
    size_t dedupe_class_bytes;
    bool dedupe_periodic;
    size_t dedupe_chunk_bytes, batch_chunk_bytes;
    int32_t dedupe_strip;
};

// A column in PIECES: a dedupe group each (uvrt_dedupe.h: 2..31 launches of one bit-identical lamp, every distinct ray traced
// once), or launches traced as they are.  The launches [k0, k0 + kc) of column g.
struct Piece {
    int g, k0, kc; bool dd; int64_t chunk_gids; DedupeGroup G;
    DedupeTally cand[DEDUPE_CLASS_MAX]; int ncand; double keys;       // its owners' multi-bit masks by sampled frequency
    int ncls, cls_base; DedupeClasses cls;                            // the classes it gets, from class plane cls_base on
    DedupePeriodic per;                                               // its period table (count 0: none)
};

struct BatchPlan {
    int64_t n_pad;
    int R;                              // deposit replicas per plane in use
    size_t plane_ints;                  // R * T
    int nstops, nsweeps;
    int ngroups;                        // the stops' lamp columns (x, z), their first physical plane and launches
    float gx[MAX_BATCH], gz[MAX_BATCH];
    int gfirst[MAX_BATCH], gsize[MAX_BATCH];
    int32_t phys[MAX_BATCH];            // logical launch -> physical plane: the stops' columns first, then the sweeps in logical order
    struct { float lx[MAX_BATCH], ly[MAX_BATCH], lz[MAX_BATCH]; uint32_t seed_prev[MAX_BATCH], seed_next[MAX_BATCH]; } gp;      // the stops, by physical plane
    struct {
        float fx[MAX_BATCH], fy[MAX_BATCH], fz[MAX_BATCH], tx[MAX_BATCH], ty[MAX_BATCH], tz[MAX_BATCH];
        uint32_t seed_prev[MAX_BATCH], seed_next[MAX_BATCH];
    } sp;                               // the sweeps, by physical plane - nstops
    uint32_t seed_after;                // SEED behind the batch
    std::vector<Piece> pieces;
    size_t dd_chunks, dd_tmp_bytes, dd_block_bytes;      // the deduped chunks, and a lane's scratch for the largest of them
    int class_cap, total_cls, cls_repl;                  // class planes: allocated behind the launch planes, dealt, replicas in use
    int per_chunk, per_sweep_chunk;                      // planes per chunk of stops traced as they are, of sweeps
};

// The chunk's key tiles and the strip of them a wave of the mark pass walks: DEDUPE_STRIP_TILES, and up to twice that where
// the chunk still keeps 4 096 waves busy -- a longer strip spreads its one search over more tiles, a shorter one leaves a
// small chunk more waves to cover each other's waits (DESIGN.md section 15 has the sweep).  Q: GenDedupeParams (uvrt_device.h);
// dedupe_strip: the developer knob, 0 = this choice.
template <class Q>
inline void mark_tiles(int32_t dedupe_strip, Q& q)
{
    dedupe_tile_range(q.g, q.g0, q.gn, DEDUPE_MARK_KEYS, q.key_lo, q.tiles);
    // ... of the key intervals that the group's period table (q.per; count 0: none) leaves to the mark pass: the tiles it
    // walks (strips of one), then the strips
    q.gaps = dedupe_periodic_gaps(q.per, q.key_lo, q.tiles * DEDUPE_MARK_KEYS, DEDUPE_MARK_KEYS, 1, q.gap_key, q.gap_keys, q.gap_strip0);
    const int64_t walked = q.gap_strip0[q.gaps];
    // (with a table few tiles are left and a wave's walk is all the pass takes: strips down to one tile)
    const int64_t fit = std::min<int64_t>(2 * DEDUPE_STRIP_TILES, std::max<int64_t>(q.per.count > 0 ? 1 : DEDUPE_STRIP_TILES, walked / 4096));
    q.strip_tiles = dedupe_strip > 0 ? dedupe_strip : (int32_t)fit;
    q.gaps = dedupe_periodic_gaps(q.per, q.key_lo, q.tiles * DEDUPE_MARK_KEYS, DEDUPE_MARK_KEYS, q.strip_tiles, q.gap_key, q.gap_keys, q.gap_strip0);
}

// Class planes dealt to the pieces by sampled frequency (Piece::cand, from dedupe_class_tally), most frequent first, at most
// `cap` of them, and every piece's class table.  A class plane's index counts from the piece's first launch plane, as a
// launch's does: the class planes lie behind the `count` launch planes, a piece's first plane is gfirst[g] + k0.  Returns the
// planes dealt.
inline int deal_classes(std::vector<Piece>& pieces, int cap, int count, const int* gfirst)
{
    int total_cls = 0;
    while (total_cls < cap) {
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
        dedupe_classes_fill(pc.cls, masks, pc.ncls, (uint32_t)(count - (gfirst[pc.g] + pc.k0) + base));
        base += pc.ncls;
    }
    return total_cls;
}

// a refusal of plan_batch: its text (the caller puts its own name in front), UVRT_ERR_INVALID
inline int plan_refuse(const char** why, const char* fmt, ...)
{
    static thread_local char text[256];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(text, sizeof text, fmt, ap);
    va_end(ap);
    *why = text;
    return UVRT_ERR_INVALID;
}

// the stops grouped by lamp column (x, z) -- the per-launch node-pair records depend on it only -- the physical planes, and
// the SEED chain in logical order
inline void plan_columns(const BatchKnobs& kn, const uvrt_launch* launches, float light_length, int count, BatchPlan& P)
{
    int group_of[MAX_BATCH];
    for (int k = 0; k < count; ++k) {
        if (launches[k].kind != UVRT_LAUNCH_STOP) continue;
        const float* lamp = launches[k].from;
        int g = 0;
        for (; g < P.ngroups; ++g)
            if (memcmp(&P.gx[g], &lamp[0], 4) == 0 && memcmp(&P.gz[g], &lamp[2], 4) == 0) break;
        if (g == P.ngroups) { P.gx[g] = lamp[0]; P.gz[g] = lamp[2]; ++P.ngroups; }
        group_of[k] = g;
        ++P.gsize[g];
    }
    for (int g = 0, acc = 0; g < P.ngroups; ++g) { P.gfirst[g] = acc; acc += P.gsize[g]; }
    int fill[MAX_BATCH] = {}, sfill = 0;
    uint32_t seed = kn.seed;
    for (int k = 0; k < count; ++k) {                    // logical order: the SEED chain
        const uvrt_launch& l = launches[k];
        if (l.kind == UVRT_LAUNCH_STOP) {
            const int g = group_of[k], ph = P.gfirst[g] + fill[g]++;
            P.phys[k] = ph;
            P.gp.lx[ph] = l.from[0]; P.gp.ly[ph] = l.from[1]; P.gp.lz[ph] = l.from[2];
            P.gp.seed_prev[ph] = seed;
            seed = uvrt_seed_next_mode(l.from, light_length, seed, kn.seed_mode);
            P.gp.seed_next[ph] = seed;
        } else {
            const int j = sfill++;
            P.phys[k] = P.nstops + j;
            P.sp.fx[j] = l.from[0]; P.sp.fy[j] = l.from[1]; P.sp.fz[j] = l.from[2];
            P.sp.tx[j] = l.to[0]; P.sp.ty[j] = l.to[1]; P.sp.tz[j] = l.to[2];
            P.sp.seed_prev[j] = seed;
            seed = uvrt_seed_next_sweep(l.from, light_length, seed);
            P.sp.seed_next[j] = seed;
        }
    }
    P.seed_after = seed;                // committed with the batch: a failed call leaves the SEED chain where it was
}

// The columns in pieces.  Launches are traced as they are in a column of one, with lamps that differ in y, with a range or a
// lamp outside dedupe_group_ok, and without BatchKnobs::may_dedupe (uvrt_set_dedupe(0), a kernel variant other than the
// default's code -- the deduped kernel exists for leaf period 2 with the LDS cache only -- the developer build's skip-generate
// probe).  A longer column is split evenly (33 launches: 17 + 16).
inline void plan_pieces(const BatchKnobs& kn, int64_t first_gid, int64_t n, BatchPlan& P)
{
    for (int g = 0; g < P.ngroups; ++g) {
        const int gfirst = P.gfirst[g], gsize = P.gsize[g];
        bool same_lamp = kn.may_dedupe && gsize >= 2;
        for (int j = 1; same_lamp && j < gsize; ++j) same_lamp = memcmp(&P.gp.ly[gfirst], &P.gp.ly[gfirst + j], 4) == 0;
        const int npieces = same_lamp ? (gsize + DEDUPE_MAX - 1) / DEDUPE_MAX : 1;
        for (int i = 0, k0 = 0; i < npieces; ++i) {
            Piece pc;
            memset(&pc, 0, sizeof pc);
            pc.g = g; pc.k0 = k0; pc.kc = gsize / npieces + (i < gsize % npieces);      // (64 launches: 22 + 21 + 21)
            k0 += pc.kc;
            const int ph0 = gfirst + pc.k0;
            if (same_lamp && pc.kc >= 2) {
                DedupeGroup& G = pc.G;
                G.lx = P.gp.lx[ph0]; G.ly = P.gp.ly[ph0]; G.lz = P.gp.lz[ph0];
                G.seed_mode = kn.seed_mode;
                G.count = pc.kc;
                G.first_gid = first_gid; G.n = n;
                for (int j = 0; j < pc.kc; ++j) { G.seed_prev[j] = P.gp.seed_prev[ph0 + j]; G.seed_next[j] = P.gp.seed_next[ph0 + j]; }
                pc.dd = dedupe_group_ok(G);
            }
            if (pc.dd) {
                // a chunk: a gid range across all the piece's launches, sized by its upper bound (no duplicates)
                pc.chunk_gids = std::max<int64_t>(64, (int64_t)(kn.dedupe_chunk_bytes / ((size_t)pc.kc * 16)) / 64 * 64);
                // ... and the range dealt evenly over that many chunks (a short last chunk leaves one lane idle at the end)
                const int64_t nch = (n + pc.chunk_gids - 1) / pc.chunk_gids;
                pc.chunk_gids = ((n + nch - 1) / nch + 63) / 64 * 64;
                const int64_t gn = std::min(pc.chunk_gids, n);
                P.dd_chunks += (size_t)((n + pc.chunk_gids - 1) / pc.chunk_gids);
                P.dd_tmp_bytes = std::max(P.dd_tmp_bytes, (size_t)pc.kc * (size_t)gn * 4);
                P.dd_block_bytes = std::max(P.dd_block_bytes, (size_t)pc.kc * (size_t)((gn + 255) / 256) * 4);
            }
            P.pieces.push_back(pc);
        }
    }
}

// The mask classes of the dedupe groups (uvrt_dedupe.h "mask classes"): every group's candidates from a sample of its key
// tiles and the class planes dealt to the groups (deal_classes).  The planes sit behind the launch planes, at most class_cap
// of them: the set's byte budget, one bit each in ReplayParams::class_of, every offset below 2^32.  Then the groups' period
// tables (uvrt_dedupe.h "period table"), words through the classes just dealt.  Both are functions of the group alone, built
// here at every call with no word from the device; the tables travel in the kernels' arguments.
inline void plan_group_tables(const BatchKnobs& kn, int count, BatchPlan& P)
{
    P.cls_repl = std::max(1, std::min(kn.dedupe_class_replicas, P.R));
    if (P.dd_chunks == 0) return;
    std::vector<uint32_t> table((size_t)DEDUPE_TILE_KEYS);
    if (kn.dedupe_classes > 0) {
        const uint64_t room = (((uint64_t)1 << 32) - 1) / (uint64_t)P.plane_ints;
        P.class_cap = (int)std::min<uint64_t>({(uint64_t)MAX_CLASS_PLANES, (uint64_t)(kn.dedupe_class_bytes / (P.plane_ints * 4)),
                                               room > (uint64_t)count ? room - (uint64_t)count : 0});
        for (Piece& pc : P.pieces)
            if (pc.dd && pc.kc <= DEDUPE_CLASS_LAUNCHES)
                pc.ncand = dedupe_class_tally(pc.G, table.data(), pc.cand, kn.dedupe_classes, &pc.keys);
        P.total_cls = deal_classes(P.pieces, P.class_cap, count, P.gfirst);
    }
    if (kn.dedupe_periodic)
        for (Piece& pc : P.pieces)
            if (pc.dd) dedupe_periodic_build(pc.G, pc.cls, table.data(), pc.per);
}

// The plan of uvrt_trace_batch / uvrt_trace_batch_launches for `count` launches over the global ids [first_gid, first_gid + n):
// UVRT_OK, or UVRT_ERR_INVALID with *why = what is wrong with the arguments (a text that lasts until the thread's next refusal).
inline int plan_batch(const BatchKnobs& kn, const uvrt_launch* launches, float light_length, int count, int64_t first_gid, int64_t n,
                      BatchPlan& P, const char** why)
{
    if (count <= 0 || count > MAX_BATCH) return plan_refuse(why, "count must be in [1,%d]", MAX_BATCH);
    if (n <= 0 || first_gid < 0 || first_gid + n > (int64_t)INT32_MAX) return plan_refuse(why, "bad global-id range");
    P = BatchPlan{};
    for (int k = 0; k < count; ++k) {
        if (launches[k].kind != UVRT_LAUNCH_STOP && launches[k].kind != UVRT_LAUNCH_SWEEP)
            return plan_refuse(why, "launch %d: kind must be UVRT_LAUNCH_STOP or UVRT_LAUNCH_SWEEP", k);
        P.nsweeps += launches[k].kind == UVRT_LAUNCH_SWEEP;
    }
    if (P.nsweeps > 0 && kn.seed_mode != 0)
        return plan_refuse(why, "seed mode 1 models the SEED race of generate.cl only; a sweep needs uvrt_set_seed_mode(ctx, 0)");
    P.nstops = count - P.nsweeps;
    P.n_pad = (n + 63) / 64 * 64;
    // deposit replicas per plane: the contention on a hot triangle's counter grows with the rays per plane
    // (16 replicas for 2 M rays), and every replica is read and zeroed again by the replay -- a shard of a launch
    // gets by with 8 (one per XCD)
    // (a fused batch is happiest with 8-12 replicas even at 2 M rays per plane: +0.4 % over 16, profiles/r03/r03_knobs_room.txt;
    // the per-launch path keeps the context's 16)
    P.R = std::min(kn.replicas, 12);
    if ((int64_t)P.R * 131072 > 2 * n) P.R = std::min(kn.replicas, 8);
    if ((uint64_t)count * (uint64_t)P.n_pad >= ((uint64_t)1 << 30) || (uint64_t)count * (uint64_t)P.R * (uint64_t)kn.T >= ((uint64_t)1 << 32))
        return plan_refuse(why, "%d launches x %lld rays exceed one batch (2^30 ray slots, 2^32 counters)", count, (long long)n);
    P.plane_ints = (size_t)P.R * (size_t)kn.T;
    plan_columns(kn, launches, light_length, count, P);
    plan_pieces(kn, first_gid, n, P);
    plan_group_tables(kn, count, P);
    // Launches traced as they are go in CHUNKS of a few planes: a chunk's rays (16 B each; a sweep's 24 B with its origins) are
    // sized to stay in the Infinity Cache between the generate that writes them and the extend that reads them.
    // (a plane's offset shares its register with the exact-step flag, PLANE_OFF6: a chunk's planes stay below 2^31 counters)
    const size_t planes_31 = std::max<size_t>(1, (((size_t)1 << 31) - 1) / P.plane_ints);
    P.per_chunk = (int)std::min(planes_31, std::max<size_t>(1, kn.batch_chunk_bytes / ((size_t)P.n_pad * 16)));
    P.per_sweep_chunk = (int)std::min(planes_31, std::max<size_t>(1, kn.batch_chunk_bytes / ((size_t)P.n_pad * 24)));
    return UVRT_OK;
}

}  // namespace uvrt

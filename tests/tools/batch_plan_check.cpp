// Developer check (no GPU): the host-only plan of a batch (csrc/uvrt_batch_plan.h) as a stand-alone program, for
// tests/test_batch_plan_cpu.py and for a sanitizer build -- the plan is integer arithmetic with edge cases (33 launches in 17 +
// 16, chunk rounding, class caps, offsets below 2^32 and 2^31).  The two SEED functions of include/uvrt.h are stand-ins here:
// the plan only chains them.  plan_batch runs over a grid of launch lists, ranges and knobs, and every plan is held to the
// invariants the emitters of uvrt_capi_batch.hip rely on; then the refusals.  Prints a tally; exit status 1 on any breach.//
//   g++ -O1 -g -std=c++17 -ffp-contract=off -fsanitize=address,undefined -fno-sanitize-recover=all
//       -I small-project-uv-robot-ray-tracer_amd/csrc tests/tools/batch_plan_check.cpp -o check && ./check
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

#include "uvrt_batch_plan.h"

using namespace uvrt;

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }
static uint32_t mix(uint32_t v) { v ^= v >> 16; v *= 0x7feb352du; v ^= v >> 15; v *= 0x846ca68bu; v ^= v >> 16; return v; }
extern "C" uint32_t uvrt_seed_next_mode(const float p[3], float, uint32_t seed_prev, int32_t seed_mode)
{
    return mix(seed_prev + 0x9E3779B9u * (bits(p[0]) ^ mix(bits(p[1])) ^ mix(mix(bits(p[2])))) + (uint32_t)seed_mode);
}
extern "C" uint32_t uvrt_seed_next_sweep(const float p[3], float, uint32_t seed_prev)
{
    return mix(seed_prev ^ 0x5bd1e995u) + bits(p[0]) + 3u * bits(p[1]) + 5u * bits(p[2]);
}

// the A, B and A2 pool of tests/batch_sequences.py: lamps 0 and 5 of the golden route, and A raised by 0.37
static const float LAMP_A[3] = {-0x1.051f12p-2f, -0x1.fdb008p-1f, -0x1.a85178p+1f};
static const float LAMP_B[3] = {-0x1.5c294cp-1f, -0x1.fdb008p-1f, -0x1.b333b2p-1f};
static const float LAMP_A2[3] = {-0x1.051f12p-2f, -0x1.403f64p-1f, -0x1.a85178p+1f};

static int g_bad = 0;
static std::string g_case;
#define CHECK(cond)                                                                          \
    do {                                                                                     \
        if (!(cond)) { if (++g_bad <= 40) printf("BREACH %s: %s (line %d)\n", g_case.c_str(), #cond, __LINE__); } \
    } while (0)

// GenDedupeParams' fields that mark_tiles reads and writes
struct MarkQ {
    DedupeGroup g; DedupePeriodic per; int64_t g0, gn, key_lo, tiles; int32_t strip_tiles, gaps;
    int32_t gap_key[DEDUPE_PERIODIC_STRATA + 1]; uint32_t gap_keys[DEDUPE_PERIODIC_STRATA + 1]; int32_t gap_strip0[DEDUPE_PERIODIC_STRATA + 2];
};

// pattern 0..2: one column of A; A and B in turn; A and A2 in turn (one column, lamps differ in y: no group); 3..5: each with a
// sweep after every third stop; 6: sweeps only
static std::vector<uvrt_launch> launches_of(int pattern, int count)
{
    std::vector<uvrt_launch> out((size_t)count);
    int stops = 0;
    for (int k = 0; k < count; ++k) {
        uvrt_launch& l = out[(size_t)k];
        memset(&l, 0, sizeof l);
        const bool sweep = pattern == 6 || (pattern >= 3 && k % 4 == 3);
        const float* a = LAMP_A;
        const float* b = pattern % 3 == 1 ? LAMP_B : (pattern % 3 == 2 ? LAMP_A2 : LAMP_A);
        if (sweep) {
            l.kind = UVRT_LAUNCH_SWEEP;
            memcpy(l.from, k & 1 ? LAMP_B : LAMP_A2, 12);
            memcpy(l.to, k & 1 ? LAMP_A : LAMP_B, 12);
        } else {
            l.kind = UVRT_LAUNCH_STOP;
            memcpy(l.from, stops++ & 1 ? b : a, 12);
        }
    }
    return out;
}

static void check_plan(const BatchKnobs& kn, const std::vector<uvrt_launch>& L, float light_length, int64_t first, int64_t n, const BatchPlan& P)
{
    const int count = (int)L.size();
    // the physical planes: a permutation; stops below nstops, each column contiguous and in logical order; sweeps behind them
    // in logical order.  The SEED chain: a sequential walk in logical order
    bool seen[MAX_BATCH] = {};
    uint32_t seed = kn.seed;
    int sweeps = 0;
    for (int k = 0; k < count; ++k) {
        const int ph = P.phys[k];
        CHECK(ph >= 0 && ph < count && !seen[ph]);
        if (ph < 0 || ph >= count) return;
        seen[ph] = true;
        const uvrt_launch& l = L[(size_t)k];
        if (l.kind == UVRT_LAUNCH_STOP) {
            CHECK(ph < P.nstops);
            int g = 0;
            while (g < P.ngroups && !(ph >= P.gfirst[g] && ph < P.gfirst[g] + P.gsize[g])) ++g;
            CHECK(g < P.ngroups);
            if (g == P.ngroups) return;
            CHECK(bits(P.gx[g]) == bits(l.from[0]) && bits(P.gz[g]) == bits(l.from[2]));
            for (int k2 = 0; k2 < k; ++k2)      // an earlier stop of the column lies below this one
                if (L[(size_t)k2].kind == UVRT_LAUNCH_STOP && bits(L[(size_t)k2].from[0]) == bits(l.from[0]) && bits(L[(size_t)k2].from[2]) == bits(l.from[2]))
                    CHECK(P.phys[k2] < ph && P.phys[k2] >= P.gfirst[g]);
            CHECK(bits(P.gp.lx[ph]) == bits(l.from[0]) && bits(P.gp.ly[ph]) == bits(l.from[1]) && bits(P.gp.lz[ph]) == bits(l.from[2]));
            CHECK(P.gp.seed_prev[ph] == seed);
            seed = uvrt_seed_next_mode(l.from, light_length, seed, kn.seed_mode);
            CHECK(P.gp.seed_next[ph] == seed);
        } else {
            const int j = sweeps++;
            CHECK(ph == P.nstops + j);
            CHECK(bits(P.sp.fx[j]) == bits(l.from[0]) && bits(P.sp.fy[j]) == bits(l.from[1]) && bits(P.sp.fz[j]) == bits(l.from[2]));
            CHECK(bits(P.sp.tx[j]) == bits(l.to[0]) && bits(P.sp.ty[j]) == bits(l.to[1]) && bits(P.sp.tz[j]) == bits(l.to[2]));
            CHECK(P.sp.seed_prev[j] == seed);
            seed = uvrt_seed_next_sweep(l.from, light_length, seed);
            CHECK(P.sp.seed_next[j] == seed);
        }
    }
    CHECK(P.seed_after == seed && sweeps == P.nsweeps && P.nstops + P.nsweeps == count);
    int in_groups = 0;
    for (int g = 0; g < P.ngroups; ++g) { CHECK(P.gfirst[g] == in_groups && P.gsize[g] >= 1); in_groups += P.gsize[g]; }
    CHECK(in_groups == P.nstops);
    // sizes, and the limits the emitters' offsets stay below: 2^30 ray slots, 2^32 counters, 2^31 counters within a chunk
    CHECK(P.n_pad >= n && P.n_pad < n + 64 && P.n_pad % 64 == 0);
    CHECK(P.R >= 1 && P.R <= kn.replicas && P.plane_ints == (size_t)P.R * (size_t)kn.T);
    const uint64_t slots = (uint64_t)count * (uint64_t)P.n_pad;
    CHECK(slots < ((uint64_t)1 << 30));
    CHECK(P.total_cls >= 0 && P.total_cls <= P.class_cap && P.class_cap <= MAX_CLASS_PLANES);
    CHECK(((uint64_t)count + (uint64_t)P.class_cap) * (uint64_t)P.plane_ints <= (((uint64_t)1 << 32) - 1) || P.class_cap == 0);
    CHECK((uint64_t)count * (uint64_t)P.plane_ints < ((uint64_t)1 << 32));
    CHECK(P.cls_repl >= 1 && P.cls_repl <= std::max(1, P.R));
    CHECK(P.per_chunk >= 1 && P.per_sweep_chunk >= 1);
    CHECK((uint64_t)(P.per_chunk - 1) * (uint64_t)P.plane_ints < ((uint64_t)1 << 31));
    CHECK((uint64_t)(P.per_sweep_chunk - 1) * (uint64_t)P.plane_ints < ((uint64_t)1 << 31));
    // the pieces: a partition of every column, deduped ones of 2..31 launches, sizes within one of each other
    size_t at = 0, dd_chunks = 0;
    int cls_next = 0;
    for (int g = 0; g < P.ngroups; ++g) {
        int k0 = 0, kmin = MAX_BATCH, kmax = 0;
        for (; at < P.pieces.size() && P.pieces[at].g == g; ++at) {
            const Piece& pc = P.pieces[at];
            CHECK(pc.k0 == k0 && pc.kc >= 1);
            k0 += pc.kc;
            kmin = std::min(kmin, pc.kc);
            kmax = std::max(kmax, pc.kc);
            const int ph0 = P.gfirst[g] + pc.k0;
            CHECK(pc.cls_base == cls_next && pc.ncls >= 0 && pc.ncls == pc.cls.count);      // no two pieces share a class plane
            cls_next += pc.ncls;
            if (!pc.dd) {
                CHECK(pc.ncls == 0 && pc.per.count == 0);
                continue;
            }
            CHECK(kn.may_dedupe && pc.kc >= 2 && pc.kc <= DEDUPE_MAX && pc.G.count == pc.kc && pc.G.first_gid == first && pc.G.n == n);
            for (int j = 0; j < pc.kc; ++j) CHECK(pc.G.seed_prev[j] == P.gp.seed_prev[ph0 + j] && pc.G.seed_next[j] == P.gp.seed_next[ph0 + j]);
            // its chunks: [0, n) in multiples of 64 gids except the last; the scratch covers the largest; the rays stay in its planes
            CHECK(pc.chunk_gids >= 64 && pc.chunk_gids % 64 == 0);
            bool first_chunk = true;
            for (int64_t g0 = 0; g0 < n; g0 += pc.chunk_gids) {
                const int64_t gn = std::min(pc.chunk_gids, n - g0);
                ++dd_chunks;
                CHECK(gn > 0 && (gn % 64 == 0 || g0 + gn == n));
                CHECK(P.dd_tmp_bytes >= (size_t)pc.kc * (size_t)gn * 4);
                CHECK(P.dd_block_bytes >= (size_t)pc.kc * (size_t)((gn + 255) / 256) * 4);
                CHECK((uint64_t)ph0 * (uint64_t)P.n_pad + (uint64_t)pc.kc * (uint64_t)(g0 + gn) <= (uint64_t)(ph0 + pc.kc) * (uint64_t)P.n_pad);
                if (first_chunk) {      // the mark pass's tiles of one chunk per piece
                    MarkQ q;
                    memset(&q, 0, sizeof q);
                    q.g = pc.G; q.per = pc.per; q.g0 = first + g0; q.gn = gn;
                    mark_tiles(kn.dedupe_strip, q);
                    CHECK(q.tiles >= 1 && q.strip_tiles >= 1 && q.gaps >= 0 && q.gaps <= DEDUPE_PERIODIC_STRATA + 1 && q.gap_strip0[0] == 0);
                    for (int i = 0; i < q.gaps; ++i) CHECK(q.gap_strip0[i + 1] > q.gap_strip0[i] && q.gap_keys[i] > 0u);
                    first_chunk = false;
                }
            }
            // every class word, in the class table and in the period table, names a class plane of this piece: counted from
            // the piece's first plane it lands in [count, count + total_cls)
            CHECK(pc.ncls <= pc.ncand && (pc.ncls == 0 || pc.kc <= DEDUPE_CLASS_LAUNCHES));
            int words = 0;
            const auto class_word = [&](uint32_t w) {
                const int plane = ph0 + (int)(w & DEDUPE_PLANE_INDEX);
                CHECK(plane >= count + pc.cls_base && plane < count + pc.cls_base + pc.ncls && plane < count + P.total_cls);
                ++words;
            };
            for (int s = 0; s < DEDUPE_CLASS_SLOTS; ++s)
                if (pc.cls.slot_mask[s] != 0u) {
                    CHECK((pc.cls.slot_word[s] & (DEDUPE_PLANE_FORM | DEDUPE_CLASS_FORM)) == (DEDUPE_PLANE_FORM | DEDUPE_CLASS_FORM));
                    class_word(pc.cls.slot_word[s]);
                }
            CHECK(words == pc.ncls);
            for (int s = 0; s < pc.per.count; ++s)
                for (int e = 0; e < pc.kc * pc.per.period[s]; ++e) {
                    const uint32_t w = pc.per.words[pc.per.word_off[s] + e];
                    if (pc.ncls > 0 && (w & DEDUPE_PLANE_FORM) && (w & DEDUPE_CLASS_FORM)) class_word(w);
                }
            CHECK(kn.dedupe_periodic || pc.per.count == 0);
        }
        CHECK(k0 == P.gsize[g] && kmax - kmin <= 1);
    }
    CHECK(at == P.pieces.size() && cls_next == P.total_cls && dd_chunks == P.dd_chunks);
    CHECK(P.dd_chunks > 0 || (P.dd_tmp_bytes == 0 && P.dd_block_bytes == 0 && P.total_cls == 0));
    CHECK(kn.dedupe_classes > 0 || P.total_cls == 0);
}

int main()
{
    const int counts[] = {1, 2, 3, 17, 31, 32, 33, 62, 63, 64};
    const int64_t ns[] = {1, 63, 64, 65, 4096, 20001}, firsts[] = {0, 3, 1200000};
    const int classes[] = {0, 1, 4, 32};
    const float light_length = 1.0f;
    BatchKnobs base = {};
    base.seed = 0x1234u; base.replicas = 16; base.may_dedupe = true;
    base.dedupe_class_replicas = 4; base.dedupe_class_bytes = (size_t)96 << 20; base.dedupe_periodic = true;
    base.dedupe_chunk_bytes = (size_t)192 << 20; base.batch_chunk_bytes = (size_t)96 << 20;
    long plans = 0, refused_size = 0, with_classes = 0, with_tables = 0, dd_pieces = 0, many_chunks = 0;
    // budgets: the defaults; then once each so small that several chunks, or no class plane, arise; triangles: a room's, and
    // so many that the counters' limits bind
    for (int budget = 0; budget < 4; ++budget)
        for (int32_t T : {54321, 30000000})
            for (int count : counts)
                for (int pattern = 0; pattern < 7; ++pattern)
                    for (int64_t n : ns)
                        for (int64_t first : firsts)
                            for (int mode = 0; mode < 2; ++mode)
                                for (int cls : classes) {
                                    if (T != 54321 && (budget != 0 || cls == 1)) continue;
                                    BatchKnobs kn = base;
                                    kn.T = T; kn.seed_mode = mode; kn.dedupe_classes = cls;
                                    if (budget == 1) kn.dedupe_chunk_bytes = 1;      // deduped chunks of 64 gids
                                    if (budget == 2) kn.batch_chunk_bytes = 1;       // one plane per chunk
                                    if (budget == 3) kn.dedupe_class_bytes = 0;      // no class plane
                                    const std::vector<uvrt_launch> L = launches_of(pattern, count);
                                    int nsweeps = 0;
                                    for (const uvrt_launch& l : L) nsweeps += l.kind == UVRT_LAUNCH_SWEEP;
                                    char name[160];
                                    snprintf(name, sizeof name, "budget %d T %d count %d pattern %d n %lld first %lld mode %d classes %d", budget, (int)T,
                                             count, pattern, (long long)n, (long long)first, mode, cls);
                                    g_case = name;
                                    BatchPlan P;
                                    const char* why = nullptr;
                                    const int rc = plan_batch(kn, L.data(), light_length, count, first, n, P, &why);
                                    ++plans;
                                    if (nsweeps > 0 && mode == 1) { CHECK(rc == UVRT_ERR_INVALID && why && strstr(why, "seed mode 1")); continue; }
                                    const int R = (int64_t)std::min(16, 12) * 131072 > 2 * n ? 8 : 12;
                                    if ((uint64_t)count * (uint64_t)((n + 63) / 64 * 64) >= ((uint64_t)1 << 30) || (uint64_t)count * (uint64_t)R * (uint64_t)T >= ((uint64_t)1 << 32)) {
                                        CHECK(rc == UVRT_ERR_INVALID && why && strstr(why, "exceed one batch"));
                                        ++refused_size;
                                        continue;
                                    }
                                    CHECK(rc == UVRT_OK);
                                    if (rc != UVRT_OK) continue;
                                    check_plan(kn, L, light_length, first, n, P);
                                    with_classes += P.total_cls > 0;
                                    for (const Piece& pc : P.pieces) { dd_pieces += pc.dd; with_tables += pc.per.count > 0; many_chunks += pc.dd && pc.chunk_gids < n; }
                                    if (budget == 1) for (const Piece& pc : P.pieces) CHECK(!pc.dd || pc.chunk_gids == 64);
                                    if (budget == 2) CHECK(P.per_chunk == 1 && P.per_sweep_chunk == 1);
                                    if (budget == 3) CHECK(P.class_cap == 0 && P.total_cls == 0);
                                    if (pattern % 3 == 2 || pattern == 6) for (const Piece& pc : P.pieces) CHECK(!pc.dd);
                                    if (pattern == 0 && count >= 2) for (const Piece& pc : P.pieces) CHECK(pc.dd);
                                    if (pattern == 0 && count == 33) CHECK(P.pieces.size() == 2 && P.pieces[0].kc == 17 && P.pieces[1].kc == 16);
                                    if (pattern == 0 && count == 64) CHECK(P.pieces.size() == 3 && P.pieces[0].kc == 22 && P.pieces[1].kc == 21 && P.pieces[2].kc == 21);
                                }
    // without dedupe no piece is a group
    {
        BatchKnobs kn = base;
        kn.T = 54321; kn.may_dedupe = false; kn.dedupe_classes = 32;
        const std::vector<uvrt_launch> L = launches_of(0, 33);
        g_case = "no dedupe";
        BatchPlan P;
        const char* why = nullptr;
        CHECK(plan_batch(kn, L.data(), light_length, 33, 0, 4096, P, &why) == UVRT_OK);
        check_plan(kn, L, light_length, 0, 4096, P);
        CHECK(P.pieces.size() == 1 && !P.pieces[0].dd && P.dd_chunks == 0);
    }
    // the refusals: their code, and a text
    {
        BatchKnobs kn = base;
        kn.T = 54321; kn.dedupe_classes = 32;
        std::vector<uvrt_launch> L = launches_of(3, 65);
        BatchPlan P;
        const char* why = nullptr;
        g_case = "refusals";
        CHECK(plan_batch(kn, L.data(), light_length, 0, 0, 4096, P, &why) == UVRT_ERR_INVALID && why && strstr(why, "count must be in [1,64]"));
        CHECK(plan_batch(kn, L.data(), light_length, 65, 0, 4096, P, &why) == UVRT_ERR_INVALID && strstr(why, "count must be in [1,64]"));
        CHECK(plan_batch(kn, L.data(), light_length, -1, 0, 4096, P, &why) == UVRT_ERR_INVALID);
        CHECK(plan_batch(kn, L.data(), light_length, 8, 0, 0, P, &why) == UVRT_ERR_INVALID && strstr(why, "bad global-id range"));
        CHECK(plan_batch(kn, L.data(), light_length, 8, 0, -5, P, &why) == UVRT_ERR_INVALID && strstr(why, "bad global-id range"));
        CHECK(plan_batch(kn, L.data(), light_length, 8, -1, 4096, P, &why) == UVRT_ERR_INVALID && strstr(why, "bad global-id range"));
        CHECK(plan_batch(kn, L.data(), light_length, 8, (int64_t)INT32_MAX - 4095, 4096, P, &why) == UVRT_ERR_INVALID);
        kn.seed_mode = 1;
        CHECK(plan_batch(kn, L.data(), light_length, 8, 0, 4096, P, &why) == UVRT_ERR_INVALID && strstr(why, "seed mode 1"));
        kn.seed_mode = 0;
        L[5].kind = 2;
        CHECK(plan_batch(kn, L.data(), light_length, 8, 0, 4096, P, &why) == UVRT_ERR_INVALID && strstr(why, "launch 5: kind must be"));
        CHECK(plan_batch(kn, L.data(), light_length, 5, 0, 4096, P, &why) == UVRT_OK);
        L[5].kind = UVRT_LAUNCH_STOP;
        CHECK(plan_batch(kn, L.data(), light_length, 64, 0, (int64_t)1 << 24, P, &why) == UVRT_ERR_INVALID && strstr(why, "exceed one batch"));
    }
    printf("%ld plans (%ld refused for their size), %ld with class planes; %ld dedupe pieces, %ld with a period table, %ld in several chunks\n",
           plans, refused_size, with_classes, dd_pieces, with_tables, many_chunks);
    printf("%d breaches\n", g_bad);
    return g_bad != 0;
}

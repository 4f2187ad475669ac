// uvrt_dedupe.h -- which photons of a lamp column are the same photon (host and device).
//
// generate.cl:13 seeds work-item gid of a launch from an f32 sum, 17 gid + 1 + 13 lx + 7 ly + 11 lz + (SEED >> 15), converted
// to uint32 and hashed.  Above 2^24 the sum takes even values only, and SEED >> 15 moves it by less than 131 072 from launch
// to launch: launches from ONE lamp position draw mostly the same hash inputs at shifted gids.  wang_hash is a bijection, so
// equal inputs under an equal lamp are the same 16-byte ray with the same hit, and different inputs are different RNG states.
// A batch traces each distinct ray of a lamp once and deposits its hit in the plane of every launch that holds it.
//
// A dedupe group: up to DEDUPE_MAX stop launches with one bit-identical lamp, in logical order, all over the call's global-id
// range [first_gid, first_gid + n).  For occurrence (k, g) with hash input h, m_j = the number of g' in the range whose input in
// launch j is h:
//   * some m_j >= 2 (sums from 2^27 on, or seed mode 1's negative sums that all convert to 0): traced alone, mask = bit k;
//   * else some j < k has m_j = 1: absorbed (mask 0) -- launch j's occurrence, or an earlier one, traces it;
//   * else the owner: mask = { j : m_j = 1 }.
// Every occurrence of one h sees the same m, so the decisions agree and every (launch, gid) is deposited exactly once.
//
// The search works on the sum as an integer (`dedupe_key`): for g' >= 1 it never decreases with g' (the f32 adds and the
// conversion are monotone), so the matches of a launch are one run near (h - offset) / 17: estimate, look at the keys
// around it, walk if they do not settle it.  gid 0 reads the other SEED and is looked at on its own.  dedupe_group_ok() says when keys and hash inputs
// are the same thing: 17 gid + 1 stays an int32 and so does every key of the call.
// A launch may hold a key twice long before the ulp reaches 17: in [2^27, 2^28) the ulp is 16 and an add whose exact result
// is a tie rounds two neighbouring gids to one value (SEED >> 15 = 8 mod 16 does it).  So the multiplicities are always
// counted, never assumed.
#pragma once
#include <stdint.h>
#include <algorithm>

#if defined(__HIPCC__)
#define UVRT_HD __host__ __device__ __forceinline__
#else
#define UVRT_HD inline
#endif

namespace uvrt {

// (the batch's own limits, here for the host-only plan of a batch, uvrt_batch_plan.h, and the device structs alike)
constexpr int MAX_BATCH = 64;              // launches per uvrt_trace_batch / uvrt_replay_batch call
constexpr int MAX_CLASS_PLANES = 64;       // class planes of one batch, all its dedupe groups together (one bit each in ReplayParams::class_of)

constexpr int DEDUPE_MAX = 31;             // launches per group: bit 31 of a ray's mask is the exact-step flag
constexpr int64_t DEDUPE_GID_END = 126322567;   // 17 gid + 1 fits an int32 below this

// generate.cl:13 -- the f32 adds in source order (int threadID; work-item 0 and seed mode 1 read SEED_{k-1})
UVRT_HD float seed_sum_of(int threadID, uint32_t SEED, float lx, float ly, float lz)
{
    float acc = (float)(int)((uint32_t)threadID * 17u + 1u);      // (int arithmetic: wraps like the device's)
    acc = acc + lx * 13.0f;
    acc = acc + ly * 7.0f;
    acc = acc + lz * 11.0f;
    acc = acc + (float)(SEED >> 15);
    return acc;
}
UVRT_HD float seed_sum(int64_t gid, float lx, float ly, float lz, uint32_t seed_prev, uint32_t seed_next, int32_t seed_mode)
{
    // generate.cl:11 (int threadID)
    return seed_sum_of((int)gid, (gid == 0 || seed_mode == 1) ? seed_prev : seed_next, lx, ly, lz);
}

// what work-item gid hands to wang_hash: float -> uint through int64; seed mode 1 converts a negative sum to 0
UVRT_HD uint32_t seed_input(int64_t gid, float lx, float ly, float lz, uint32_t seed_prev, uint32_t seed_next, int32_t seed_mode)
{
    const float acc = seed_sum(gid, lx, ly, lz, seed_prev, seed_next, seed_mode);
    return (seed_mode == 1 && acc < 0.0f) ? 0u : (uint32_t)(int64_t)acc;
}

struct DedupeGroup {
    float lx, ly, lz;                      // the group's lamp
    int32_t seed_mode;
    int32_t count;                         // launches, 2..DEDUPE_MAX
    int64_t first_gid, n;                  // the call's range: where duplicates are looked for
    uint32_t seed_prev[DEDUPE_MAX], seed_next[DEDUPE_MAX];
    // filled by dedupe_group_ok:
    int32_t offset[DEDUPE_MAX];            // key of launch j ~ 17 gid + offset[j]
    int32_t key0[DEDUPE_MAX];              // key of launch j's gid 0 (first_gid == 0)
};

// the sum as an integer (an int32 within a group that dedupe_group_ok accepts); equal keys <=> equal hash inputs there
UVRT_HD int32_t dedupe_key(const DedupeGroup& G, int j, int64_t gid)
{
    const int32_t s = (int32_t)seed_sum(gid, G.lx, G.ly, G.lz, G.seed_prev[j], G.seed_next[j], G.seed_mode);
    return (G.seed_mode == 1 && s < 0) ? 0 : s;
}

// the same for a gid >= 1 (no work-item 0 among them): they all read one SEED of launch j, dedupe_seed1 (a kernel that walks
// the launches keeps it in a register)
UVRT_HD uint32_t dedupe_seed1(const DedupeGroup& G, int j) { return G.seed_mode == 1 ? G.seed_prev[j] : G.seed_next[j]; }
UVRT_HD int32_t dedupe_key1_of(const DedupeGroup& G, uint32_t seed1, int32_t gid)
{
    const int32_t s = (int32_t)seed_sum_of(gid, seed1, G.lx, G.ly, G.lz);
    return (G.seed_mode == 1 && s < 0) ? 0 : s;
}
UVRT_HD int32_t dedupe_key1(const DedupeGroup& G, int j, int32_t gid) { return dedupe_key1_of(G, dedupe_seed1(G, j), gid); }

// Where key t sits among launch j's gids >= 1 of the call's range [lo, last]: walk from the estimate g (the keys never
// decrease).  Returns the key found there (== t: a match at g).  (gids as int32: the range ends below DEDUPE_GID_END.)
UVRT_HD int32_t dedupe_find(const DedupeGroup& G, int j, int32_t t, int32_t lo, int32_t last, int32_t& g)
{
    g = g < lo ? lo : (g > last ? last : g);
    int32_t v = dedupe_key1(G, j, g);
    while (v > t && g > lo) v = dedupe_key1(G, j, --g);
    while (v < t && g < last) v = dedupe_key1(G, j, ++g);
    return v;
}
// the estimate from the key alone: key ~ 17 gid + offset[j]
UVRT_HD int32_t dedupe_estimate(const DedupeGroup& G, int j, int32_t t)
{
    return (int32_t)((float)((int64_t)t - (int64_t)G.offset[j]) * (1.0f / 17.0f));
}

// Occurrences of key t in launch j over the call's range: 0, 1, or 2 for "two or more"; g = where the key is expected.
// The keys at g and its two neighbours settle nearly every case without a loop -- a match with both its neighbours known, or
// t strictly between two of the three -- one more key settles a match at the edge of the three, the walk takes the rest.
// Nothing is assumed about how often a launch holds a key (a sum that ties in an add holds it twice well below 2^28).
UVRT_HD int dedupe_multiplicity(const DedupeGroup& G, int j, int32_t t, int32_t g)
{
    int m = 0;
    int32_t lo = (int32_t)G.first_gid;
    const int32_t last = (int32_t)(G.first_gid + G.n - 1);
    if (lo == 0) { m += G.key0[j] == t; lo = 1; }
    if (lo > last) return m;
    g = g < lo ? lo : (g > last ? last : g);
    const int32_t gm = g > lo ? g - 1 : g, gp = g < last ? g + 1 : g;
    const int32_t a = dedupe_key1(G, j, gm), b = dedupe_key1(G, j, g), c = dedupe_key1(G, j, gp);
    if (b == t) m += 1 + ((gm < g) & (a == t)) + ((gp > g) & (c == t));
    else if (a == t) m += 1 + (gm > lo && dedupe_key1(G, j, gm - 1) == t);          // (b != t: the run ends at gm)
    else if (c == t) m += 1 + (gp < last && dedupe_key1(G, j, gp + 1) == t);
    else if (!(((a < t) | (gm == lo)) & ((t < c) | (gp == last)))) {                 // t is not between the three: walk
        if (dedupe_find(G, j, t, lo, last, g) == t)
            m += 1 + ((g > lo && dedupe_key1(G, j, g - 1) == t) || (g < last && dedupe_key1(G, j, g + 1) == t));
    }
    return m > 2 ? 2 : m;
}

// the mask of occurrence (k, gid): 0 = absorbed, else the launches whose plane its hit goes to
UVRT_HD uint32_t dedupe_mask(const DedupeGroup& G, int k, int64_t gid)
{
    const int32_t t = dedupe_key(G, k, gid);
    // the copy in launch j sits (offset[k] - offset[j]) / 17 gids from this one (work-item 0 reads the other SEED: from its key)
    const int32_t here = gid == 0 ? dedupe_estimate(G, k, t) : (int32_t)gid;
    uint32_t ones = 0;
    bool many = false;
    for (int j = 0; j < G.count; ++j) {
        const int m = dedupe_multiplicity(G, j, t, here + (int32_t)((float)(G.offset[k] - G.offset[j]) * (1.0f / 17.0f)));
        many = many || m >= 2;
        if (m == 1) ones |= 1u << j;
    }
    if (many) return 1u << k;
    if ((ones & ((1u << k) - 1u)) != 0) return 0u;
    return ones;
}

// ---- The same masks from one pass per key TILE (k_dedupe_mark; uvrt_dedupe_plan_tiled runs these functions on the host) ----
// The multiplicities are a property of the key, not of the occurrence, and from gid 1 on a launch's keys never decrease: the
// occurrences of a key interval [t0, t0 + W) are ONE gid run per launch.  A tile takes a table of W entries, one per key value
// (below 2^24 every integer is a key), inserts the runs of all launches over the call's WHOLE range -- bit j = launch j holds
// the key, DEDUPE_MANY = some launch holds it twice and more -- and then reads the mask of every occurrence whose gid lies in
// the chunk from its key's entry: dedupe_mask()'s rule with m_j read from the table, K keys per gid instead of 3 K^2.
// gid 0 reads the other SEED and is outside the monotone run: it belongs to the tile that holds key0[j].
constexpr uint32_t DEDUPE_MANY = 1u << 31;     // (DEDUPE_MAX = 31 leaves the bit free)
// the host's tile (the class tally and the deposit count below); the mark pass walks narrower ones, DEDUPE_MARK_KEYS -- the
// masks do not depend on the width
constexpr int32_t DEDUPE_TILE_KEYS = 3840;

// The first gid of [lo, hi) whose key in launch j is >= t, or hi; lo >= 1.  From the estimate in doubling steps to a bracket,
// then by halves: a few keys where the estimate is good, and no long walk where it is not (seed mode 1's run of key 0).
UVRT_HD int32_t dedupe_lower_bound(const DedupeGroup& G, int j, int64_t t, int32_t lo, int32_t hi)
{
    if (lo >= hi) return hi;
    int32_t g = (int32_t)((float)(t - (int64_t)G.offset[j]) * (1.0f / 17.0f));
    g = g < lo ? lo : (g > hi - 1 ? hi - 1 : g);
    int32_t a, b;                              // key(a) < t or a == lo - 1; key(b) >= t or b == hi
    if ((int64_t)dedupe_key1(G, j, g) >= t) {
        a = lo - 1; b = g;
        for (int32_t step = 1; b > lo; step += step) {
            const int32_t q = b - lo > step ? b - step : lo;
            if ((int64_t)dedupe_key1(G, j, q) >= t) b = q; else { a = q; break; }
        }
    } else {
        a = g; b = hi;
        for (int32_t step = 1; a < hi - 1; step += step) {
            const int32_t q = hi - 1 - a > step ? a + step : hi - 1;
            if ((int64_t)dedupe_key1(G, j, q) < t) a = q; else { b = q; break; }
        }
    }
    while (b - a > 1) {
        const int32_t m = a + (b - a) / 2;
        if ((int64_t)dedupe_key1(G, j, m) >= t) b = m; else a = m;
    }
    return b;
}

// launch j's gids >= 1 of the call's range with a key in [t0, t0 + W): the run [g_lo, g_hi)
UVRT_HD void dedupe_tile_run(const DedupeGroup& G, int j, int64_t t0, int32_t W, int32_t& g_lo, int32_t& g_hi)
{
    const int32_t lo = (int32_t)(G.first_gid > 1 ? G.first_gid : 1), hi = (int32_t)(G.first_gid + G.n);
    g_lo = dedupe_lower_bound(G, j, t0, lo, hi);
    g_hi = dedupe_lower_bound(G, j, t0 + W, g_lo, hi);
}
// does the call's range hold launch j's gid 0, with its key in [t0, t0 + W)?
UVRT_HD bool dedupe_tile_holds_key0(const DedupeGroup& G, int32_t key0, int64_t t0, int32_t W)
{
    return G.first_gid == 0 && (int64_t)key0 >= t0 && (int64_t)key0 < t0 + W;
}
UVRT_HD bool dedupe_tile_holds_gid0(const DedupeGroup& G, int j, int64_t t0, int32_t W) { return dedupe_tile_holds_key0(G, G.key0[j], t0, W); }
// the table entry of a key of the tile (t0 is a key of the group: it fits an int32), or W and more for a key outside it
UVRT_HD uint32_t dedupe_tile_slot(int32_t key, int64_t t0) { return (uint32_t)key - (uint32_t)(int32_t)t0; }

// one occurrence of launch j at `slot` (the device's table is in LDS, its workgroup inserts at once)
UVRT_HD void dedupe_tile_insert(uint32_t* table, uint32_t slot, int j)
{
    const uint32_t bit = 1u << j;
#if defined(__HIP_DEVICE_COMPILE__)
    if (atomicOr(&table[slot], bit) & bit) atomicOr(&table[slot], DEDUPE_MANY);
#else
    if (table[slot] & bit) table[slot] |= DEDUPE_MANY;
    table[slot] |= bit;
#endif
}
// the mask of an occurrence of launch k from its key's entry, after every insert
UVRT_HD uint32_t dedupe_tile_resolve(uint32_t entry, int k)
{
    if (entry & DEDUPE_MANY) return 1u << k;
    if ((entry & ((1u << k) - 1u)) != 0) return 0u;
    return entry;
}

// The tiles of the chunk [c0, c0 + cn) of the call's range: they partition the keys from the smallest to the largest of any
// launch's gids in the chunk -- at the ends of the chunk (the keys never decrease from gid 1 on) and at gid 0.
UVRT_HD void dedupe_tile_range(const DedupeGroup& G, int64_t c0, int64_t cn, int32_t W, int64_t& key_lo, int64_t& tiles)
{
    int64_t kmin = INT64_MAX, kmax = INT64_MIN;
    const int64_t last = c0 + cn - 1, lo1 = c0 > 1 ? c0 : 1;
    for (int j = 0; j < G.count; ++j) {
        int64_t e[3];
        int ne = 0;
        if (c0 == 0) e[ne++] = G.key0[j];
        if (lo1 <= last) { e[ne++] = dedupe_key1(G, j, (int32_t)lo1); e[ne++] = dedupe_key1(G, j, (int32_t)last); }
        for (int i = 0; i < ne; ++i) { kmin = e[i] < kmin ? e[i] : kmin; kmax = e[i] > kmax ? e[i] : kmax; }
    }
    key_lo = kmin;
    tiles = cn > 0 ? (kmax - kmin) / W + 1 : 0;
}

// ---- Strips of narrow tiles (k_dedupe_mark: a wave owns a strip; dedupe_plan_tiled walks strips of a given length on the host) ----
// The unit that owns a tile is one wave: a table of DEDUPE_MARK_KEYS entries (about 56 gids per launch, one round of a wave)
// in 3 840 B of LDS, so four single-wave workgroups find room on a CU beside the other lane's traversal grid and none of them
// meets another at a barrier.  A unit walks a STRIP of DEDUPE_STRIP_TILES consecutive tiles and carries the run bounds: a
// tile's g_hi per launch is the next tile's g_lo, and g_hi is where the run's keys leave the tile -- found by the insert pass
// itself, which looks at the keys from g_lo on anyway (dedupe_in_tile; the keys never decrease).  Only a strip's first tile
// searches (one dedupe_lower_bound per launch).
// The insert needs no answer from the table: a launch holds a key twice exactly where two NEIGHBOURING gids of its run hold it
// (the keys never decrease from gid 1 on), so an occurrence knows from the keys at g - 1 and g + 1 whether to set
// DEDUPE_MANY (dedupe_run_twice, dedupe_tile_insert_run: one OR, nothing read back, no wait between the launches' inserts).
// gid 0 is outside the monotone run: it goes in last, with dedupe_tile_insert, which reads the entry.
constexpr int32_t DEDUPE_MARK_KEYS = 960;
constexpr int32_t DEDUPE_STRIP_TILES = 4;

// is `key`, the key of a gid >= g_lo of a launch whose run starts at g_lo, still in the tile?  (key >= t0 there)
UVRT_HD bool dedupe_in_tile(int32_t key, int64_t t0, int32_t W) { return dedupe_tile_slot(key, t0) < (uint32_t)W; }
// does the launch with dedupe_seed1 `seed1` hold `key`, the key of its gid g, at a neighbour of g among the gids [lo, hi)
// too?  lo >= 1
UVRT_HD bool dedupe_run_twice(const DedupeGroup& G, uint32_t seed1, int32_t g, int32_t key, int32_t lo, int32_t hi)
{
    const int before = (g > lo) & (dedupe_key1_of(G, seed1, g - 1) == key), after = (g + 1 < hi) & (dedupe_key1_of(G, seed1, g + 1) == key);
    return (before | after) != 0;
}
// one occurrence of launch j's run at `slot`; twice: dedupe_run_twice
UVRT_HD void dedupe_tile_insert_run(uint32_t* table, uint32_t slot, int j, bool twice)
{
    const uint32_t v = (1u << j) | (twice ? DEDUPE_MANY : 0u);
#if defined(__HIP_DEVICE_COMPILE__)
    atomicOr(&table[slot], v);
#else
    table[slot] |= v;
#endif
}
// the first gid (>= 1) of the call's range whose key in launch j is >= t0: launch j's g_lo in the tile at t0
UVRT_HD int32_t dedupe_strip_first(const DedupeGroup& G, int j, int64_t t0)
{
    return dedupe_lower_bound(G, j, t0, (int32_t)(G.first_gid > 1 ? G.first_gid : 1), (int32_t)(G.first_gid + G.n));
}

// Host: one tile's table over the keys [t0, t0 + W), as the mark pass fills it: every launch's run over the call's WHOLE range
// with dedupe_tile_insert_run, then gid 0 with dedupe_tile_insert.  A run starts at start[j] (the g_hi a strip carries from its
// previous tile; start may be g_hi itself) or, without `start`, where a search finds it, and ends where its keys leave the tile:
// g_lo / g_hi.  Returns whether some launch's gid 0 fell in the tile.
inline bool dedupe_tile_fill(const DedupeGroup& G, int64_t t0, int32_t W, const int32_t* start, uint32_t* table, int32_t* g_lo, int32_t* g_hi)
{
    const int32_t lo = (int32_t)(G.first_gid > 1 ? G.first_gid : 1), hi = (int32_t)(G.first_gid + G.n);
    for (int32_t i = 0; i < W; ++i) table[i] = 0u;
    for (int j = 0; j < G.count; ++j) {
        g_lo[j] = start ? start[j] : dedupe_strip_first(G, j, t0);
        const uint32_t seed1 = dedupe_seed1(G, j);
        int32_t g = g_lo[j];
        for (; g < hi; ++g) {
            const int32_t key = dedupe_key1_of(G, seed1, g);
            if (!dedupe_in_tile(key, t0, W)) break;
            dedupe_tile_insert_run(table, dedupe_tile_slot(key, t0), j, dedupe_run_twice(G, seed1, g, key, lo, hi));
        }
        g_hi[j] = g;
    }
    bool gid0 = false;
    for (int j = 0; j < G.count; ++j)
        if (dedupe_tile_holds_gid0(G, j, t0, W)) { dedupe_tile_insert(table, dedupe_tile_slot(G.key0[j], t0), j); gid0 = true; }
    return gid0;
}

// Host: the masks of the chunk [c0, c0 + cn) of a group's range, masks[k * cn + i], tile by tile with a table of W entries,
// in strips of `strip` tiles with carried bounds as the device walks them (the device's strip length is its launcher's choice,
// DEDUPE_STRIP_TILES and more; the masks depend on it as little as on W)
// the tiles of one key interval [key_lo, key_lo + keys): the last one is cut at the interval's end (its width w), so that the
// mark pass may walk the parts of a chunk's keys that the period table below leaves to it and nothing beyond them
inline void dedupe_plan_tiled_keys(const DedupeGroup& G, int32_t W, int32_t strip, int64_t c0, int64_t cn, int64_t key_lo, int64_t keys,
                                   uint32_t* table, uint32_t* masks)
{
    const int64_t tiles = (keys + W - 1) / W;
    int32_t g_lo[DEDUPE_MAX], g_hi[DEDUPE_MAX];
    for (int64_t tile = 0; tile < tiles; ++tile) {
        const int64_t t0 = key_lo + tile * W;
        const int32_t w = (int32_t)(keys - tile * W < W ? keys - tile * W : W);
        dedupe_tile_fill(G, t0, w, tile % strip == 0 ? nullptr : g_hi, table, g_lo, g_hi);
        for (int k = 0; k < G.count; ++k) {
            const int64_t a = g_lo[k] > c0 ? g_lo[k] : c0, b = g_hi[k] < c0 + cn ? g_hi[k] : c0 + cn;
            for (int64_t g = a; g < b; ++g)
                masks[(int64_t)k * cn + (g - c0)] = dedupe_tile_resolve(table[dedupe_tile_slot(dedupe_key1(G, k, (int32_t)g), t0)], k);
            if (c0 == 0 && dedupe_tile_holds_gid0(G, k, t0, w))
                masks[(int64_t)k * cn] = dedupe_tile_resolve(table[dedupe_tile_slot(G.key0[k], t0)], k);
        }
    }
}
inline void dedupe_plan_tiled(const DedupeGroup& G, int32_t W, int32_t strip, int64_t c0, int64_t cn, uint32_t* table, uint32_t* masks)
{
    int64_t key_lo, tiles;
    dedupe_tile_range(G, c0, cn, W, key_lo, tiles);
    dedupe_plan_tiled_keys(G, W, strip, c0, cn, key_lo, tiles * W, table, masks);
}

// ---- Mask classes: one deposit per traced ray ("mask classes") ----
// An owner deposits once per set bit of its mask, and a group's owners hold few distinct masks (71 in the headline, 32 of them
// cover 0.9995 of its owners).  Each frequent multi-bit mask gets a count plane of its own behind the launch planes of the
// batch, a ray of that mask deposits there ONCE, and the fold adds a class plane into every launch of its mask: the per-launch
// totals stay the same exact integers.  The class list is a function of the group alone -- the host tallies the owners' masks
// over a fixed sample of narrow key tiles of the call's range (dedupe_class_tally) -- and never decides correctness: a mask
// without a class keeps the per-bit deposits.
// The word a compacted ray carries instead of its mask (k_dedupe_write -> ExtendParams::masks -> retire_ray):
//   DEDUPE_PLANE_FORM | index                       a single-bit mask: the launch's own plane, index = the bit
//   DEDUPE_PLANE_FORM | DEDUPE_CLASS_FORM | index   a classed mask: its class plane, index counted from the group's first plane
//   the mask itself (bits 0..29)                    any other mask: one deposit per set bit
// Bit 31 stays the exact-step flag of the traversal's register, so a group of 31 launches (bit 30 is a launch there) takes no
// classes and keeps the masks altogether, as does every group when classes are off.
constexpr int DEDUPE_CLASS_MAX = 32;            // classes per group
constexpr int DEDUPE_CLASSES_DEFAULT = 32;      // uvrt_set_dedupe_classes' default (DESIGN.md section 15 has the measurement)
constexpr int DEDUPE_CLASS_SLOTS = 64;          // the lookup table: open addressing, at most half full
constexpr int DEDUPE_CLASS_LAUNCHES = 30;       // launches of a group that may take classes
constexpr uint32_t DEDUPE_PLANE_FORM = 1u << 30, DEDUPE_CLASS_FORM = 1u << 29, DEDUPE_PLANE_INDEX = 0xFFFFu;

struct DedupeClasses {
    int32_t count;                              // 0: every ray keeps its mask
    uint32_t mask[DEDUPE_CLASS_MAX];            // most frequent first
    uint32_t slot_mask[DEDUPE_CLASS_SLOTS];     // the table: a class's mask (0 = empty) ...
    uint32_t slot_word[DEDUPE_CLASS_SLOTS];     // ... and the word of its rays
};

UVRT_HD uint32_t dedupe_class_slot(uint32_t mask) { return (mask * 0x9E3779B1u) >> 26; }
UVRT_HD bool dedupe_single_bit(uint32_t mask) { return (mask & (mask - 1u)) == 0u; }
UVRT_HD int dedupe_popcount(uint32_t v) { return __builtin_popcount(v); }

// the word of an owner with `mask` (not 0) from the table (the device's copy is in LDS); on = the group takes classes
UVRT_HD uint32_t dedupe_deposit_word(bool on, const uint32_t* slot_mask, const uint32_t* slot_word, uint32_t mask)
{
    if (!on) return mask;
    if (dedupe_single_bit(mask)) return DEDUPE_PLANE_FORM | (uint32_t)__builtin_ctz(mask);
    for (uint32_t s = dedupe_class_slot(mask);; s = (s + 1u) & (uint32_t)(DEDUPE_CLASS_SLOTS - 1)) {
        const uint32_t m = slot_mask[s];
        if (m == mask) return slot_word[s];
        if (m == 0u) return mask;
    }
}
// atomics a ray with this word issues when it hits (on: as above -- without classes bit 30 is a launch like any other)
UVRT_HD int dedupe_word_deposits(bool on, uint32_t word) { return (on && (word & DEDUPE_PLANE_FORM)) ? 1 : dedupe_popcount(word); }

// Host: the table of a class list; class i's plane is `first_plane + i` planes from the group's first launch plane
inline void dedupe_classes_fill(DedupeClasses& C, const uint32_t* masks, int count, uint32_t first_plane)
{
    C = DedupeClasses{};
    C.count = count;
    for (int i = 0; i < count; ++i) {
        C.mask[i] = masks[i];
        uint32_t s = dedupe_class_slot(masks[i]);
        while (C.slot_mask[s] != 0u) s = (s + 1u) & (uint32_t)(DEDUPE_CLASS_SLOTS - 1);
        C.slot_mask[s] = masks[i];
        C.slot_word[s] = DEDUPE_PLANE_FORM | DEDUPE_CLASS_FORM | (first_plane + (uint32_t)i);
    }
}

// Host: the ends of a group's keys over the gids >= 1 of the call's range, [lo1, last]: the smallest first key of a launch and
// one past the largest last key
inline void dedupe_key_span(const DedupeGroup& G, int64_t lo1, int64_t last, int64_t& klo, int64_t& khi)
{
    klo = INT64_MAX;
    khi = INT64_MIN;
    for (int j = 0; j < G.count; ++j) {
        const int64_t a = dedupe_key1(G, j, (int32_t)lo1), b = (int64_t)dedupe_key1(G, j, (int32_t)last) + 1;
        klo = a < klo ? a : klo;
        khi = b > khi ? b : khi;
    }
}
// Host: the sorted cut points between a group's strata (the tally below and the period table have the reasons): every launch's
// first key of [lo1, last] and one past its last, and for the binades b_first .. b_last the boundary 2^b and 2^b + s_j of
// every launch.  `ends`: work-item 0's keys (a range from gid 0) and the range ends klo / khi, as the caller has clamped them,
// are cuts too.  `cut`: room for 3 K + (b_last - b_first + 1) (K + 1) + 2.  Returns their number.
inline int dedupe_cuts(const DedupeGroup& G, int64_t lo1, int64_t last, int b_first, int b_last, bool ends, int64_t klo, int64_t khi,
                       int64_t* cut)
{
    int ncut = 0;
    for (int j = 0; j < G.count; ++j) {
        cut[ncut++] = dedupe_key1(G, j, (int32_t)lo1);
        cut[ncut++] = (int64_t)dedupe_key1(G, j, (int32_t)last) + 1;
        if (ends && G.first_gid == 0) cut[ncut++] = G.key0[j];
    }
    if (ends) { cut[ncut++] = klo; cut[ncut++] = khi; }
    for (int b = b_first; b <= b_last; ++b) {
        const int64_t B = (int64_t)1 << b;
        cut[ncut++] = B;
        for (int j = 0; j < G.count; ++j) cut[ncut++] = B + (int64_t)(dedupe_seed1(G, j) >> 15);
    }
    std::sort(cut, cut + ncut);
    return ncut;
}

// Host: the multi-bit masks of a group's owners by frequency, from a thin sample: one narrow key tile per STRATUM of the keys.
// Which launches hold a key is periodic in the key wherever nothing about the sums changes: the keys advance by 17 per gid and
// round to a multiple of the ulp, so the pattern repeats every 17 ulp keys (34 ulp with the ties' round-to-even).  What changes
// it: a launch's first and last key of the call's range (a copy beyond them is outside the range), and a binade boundary 2^b,
// b >= 24 -- crossed by the final sum at key 2^b in every launch and by launch j's sum before its last add, the SEED term
// s_j = SEED >> 15, at key 2^b + s_j.  Between two neighbours of these 2 K + (K + 1) per-binade points the masks' shares are those of any
// two periods, so a tile of 68 ulp keys from the middle of each stratum, weighted by the stratum's length, stands for it.  (The
// lamp's terms move a boundary by a few keys and work-item 0 reads the other SEED: neither is looked for, the list decides
// no result.)  A key that no launch holds twice has ONE owner and its table entry is that owner's mask, so the tally reads
// the table and generates nothing.  Returns the distinct multi-bit masks found, most frequent first (ties: the smaller
// mask), at most `cap`; *keys = the weighted keys with an owner.  `table`: DEDUPE_TILE_KEYS entries.
struct DedupeTally { uint32_t mask; double n; };
inline int dedupe_class_tally(const DedupeGroup& G, uint32_t* table, DedupeTally* out, int cap, double* keys)
{
    constexpr uint32_t H = 512;                 // (a group of 30 launches could hold more masks: the rarest are not counted then)
    DedupeTally h[H] = {};
    uint32_t used = 0;
    double seen = 0.0;
    // the strata's bounds
    int64_t cut[3 * DEDUPE_MAX + 7 * (DEDUPE_MAX + 1) + 2];
    const int64_t last = G.first_gid + G.n - 1, lo1 = G.first_gid > 1 ? G.first_gid : 1;
    if (lo1 > last) { if (keys) *keys = 0.0; return 0; }
    int64_t klo, khi;
    dedupe_key_span(G, lo1, last, klo, khi);
    // (only the binades whose points can lie among the keys: B + 131072 <= klo holds up to some binade, B >= khi from one on)
    int b_first = 24, b_last = 30;
    while (b_first <= b_last && ((int64_t)1 << b_first) + 131072 <= klo) ++b_first;
    while (b_last >= b_first && ((int64_t)1 << b_last) >= khi) --b_last;
    const int ncut = dedupe_cuts(G, lo1, last, b_first, b_last, false, klo, khi, cut);
    int32_t g_lo[DEDUPE_MAX], g_hi[DEDUPE_MAX];
    for (int i = 0; i + 1 < ncut; ++i) {
        const int64_t a = cut[i] < klo ? klo : cut[i], b = cut[i + 1] > khi ? khi : cut[i + 1];
        if (b <= a) continue;
        int64_t ulp = 1;
        while (((int64_t)1 << 24) * ulp < b) ulp += ulp;
        int64_t W = 68 * ulp < 272 ? 272 : 68 * ulp;
        W = W > DEDUPE_TILE_KEYS ? DEDUPE_TILE_KEYS : W;
        W = W > b - a ? b - a : W;
        const double weight = (double)(b - a) / (double)W;
        dedupe_tile_fill(G, a + (b - a - W) / 2, (int32_t)W, nullptr, table, g_lo, g_hi);
        for (int32_t k = 0; k < (int32_t)W; ++k) {
            const uint32_t e = table[k];
            if (e == 0u || (e & DEDUPE_MANY)) continue;
            seen += weight;
            if (dedupe_single_bit(e)) continue;
            uint32_t at = (e * 0x9E3779B1u) >> 23;
            while (h[at].mask != 0u && h[at].mask != e) at = (at + 1u) & (H - 1u);
            if (h[at].mask == 0u) {
                if (used >= H / 2u) continue;
                ++used;
                h[at].mask = e;
            }
            h[at].n += weight;
        }
    }
    if (keys) *keys = seen;
    int n = 0;
    for (uint32_t i = 0; i < H; ++i) {          // compact, then an insertion sort: the lists are short
        if (h[i].mask != 0u) h[n++] = h[i];
    }
    for (int i = 1; i < n; ++i) {
        const DedupeTally v = h[i];
        int at = i;
        for (; at > 0 && (h[at - 1].n < v.n || (h[at - 1].n == v.n && h[at - 1].mask > v.mask)); --at) h[at] = h[at - 1];
        h[at] = v;
    }
    n = n < cap ? n : cap;
    for (int i = 0; i < n; ++i) out[i] = h[i];
    return n;
}

// Host: the atomics the owners of a group issue with this class list (count 0: classes off, one per occurrence), every tile
inline int64_t dedupe_class_deposits(const DedupeGroup& G, int32_t W, const DedupeClasses& C, uint32_t* table)
{
    int64_t key_lo, tiles, total = 0;
    dedupe_tile_range(G, G.first_gid, G.n, W, key_lo, tiles);
    int32_t g_lo[DEDUPE_MAX], g_hi[DEDUPE_MAX];
    for (int64_t tile = 0; tile < tiles; ++tile) {
        const int64_t t0 = key_lo + tile * W;
        dedupe_tile_fill(G, t0, W, nullptr, table, g_lo, g_hi);
        for (int32_t i = 0; i < W; ++i) {
            const uint32_t e = table[i];
            if (e != 0u && !(e & DEDUPE_MANY)) total += dedupe_word_deposits(C.count > 0, dedupe_deposit_word(C.count > 0, C.slot_mask, C.slot_word, e));
        }
        // a key that some launch holds twice: every occurrence is its own owner with its own bit
        for (int j = 0; j < G.count; ++j) {
            for (int32_t g = g_lo[j]; g < g_hi[j]; ++g) total += (table[dedupe_tile_slot(dedupe_key1(G, j, g), t0)] & DEDUPE_MANY) != 0u;
            if (dedupe_tile_holds_gid0(G, j, t0, W)) total += (table[dedupe_tile_slot(G.key0[j], t0)] & DEDUPE_MANY) != 0u;
        }
    }
    return total;
}

// Host: may these launches form a group?  Fills G.offset and G.key0.  No: a lamp that is not finite, a range past
// DEDUPE_GID_END, or a sum that leaves the int32 range.
inline bool dedupe_group_ok(DedupeGroup& G)
{
    if (G.count < 2 || G.count > DEDUPE_MAX || G.n <= 0 || G.first_gid < 0 || G.first_gid + G.n > DEDUPE_GID_END) return false;
    const float big = 1e7f;
    if (!(G.lx > -big && G.lx < big) || !(G.ly > -big && G.ly < big) || !(G.lz > -big && G.lz < big)) return false;
    const int64_t last = G.first_gid + G.n - 1, lo1 = G.first_gid > 1 ? G.first_gid : 1, at = lo1 <= last ? lo1 : last;
    const auto sum64 = [&](int j, int64_t gid) {
        return (int64_t)seed_sum(gid, G.lx, G.ly, G.lz, G.seed_prev[j], G.seed_next[j], G.seed_mode);
    };
    // the sums of a launch never decrease from gid 1 on: its extremes are at the ends of the range (and at gid 0)
    int64_t smin = INT64_MAX, smax = INT64_MIN;
    for (int j = 0; j < G.count; ++j) {
        const int64_t ends[3] = {sum64(j, G.first_gid), sum64(j, at), sum64(j, last)};
        for (int64_t e : ends) { smin = e < smin ? e : smin; smax = e > smax ? e : smax; }
    }
    if (smin <= (int64_t)INT32_MIN + 1 || smax >= (int64_t)INT32_MAX - 1) return false;
    for (int j = 0; j < G.count; ++j) {
        // (from the sum itself: seed mode 1's zero for a negative sum says nothing about where the positive ones lie)
        G.offset[j] = (int32_t)(sum64(j, at) - 17 * at);
        G.key0[j] = dedupe_key(G, j, 0);
    }
    return true;
}

// ---- Interior masks from a per-stratum period table ("period table") ----
// Which launches hold a key is an exact periodic function of the key away from a few events, and so is the mask of an
// occurrence as a function of its gid: mask(k, g) = words[stratum][k][g mod P].  The host finds the strata and builds the
// tables (dedupe_periodic_build), the mark pass walks only the keys outside them (dedupe_periodic_gaps), the write pass reads
// an interior occurrence's word from the table (dedupe_periodic_word) and the owners per block of gids come from it in closed
// form (dedupe_periodic_owners).  dedupe_mask() stays the definition; uvrt_dedupe_plan_periodic runs these functions on the
// CPU.
//
// The sums.  For gid g >= 1 of launch j: a0 = fl(17 g + 1), a1 = fl(a0 + c1), a2 = fl(a1 + c2), a3 = fl(a2 + c3),
// a4 = fl(a3 + s_j), key = trunc(a4), with the lamp's terms c and s_j = SEED_j >> 15 (an integer below 2^17).
// Let REGION be a set of gids of launch j over which each of a0..a4 stays positive and inside ONE binade of its own, with ulps
// u0..u4 <= u, and P a multiple of 2 max(u, 1).  Then for g and g + P in the region every a_i(g + P) = a_i(g) + 17 P: the
// exact argument of each rounding moves by 17 P, a multiple of 2 u_i, so its place on the binade's grid AND the parity that
// decides a tie stay the same (this is why P takes 2 u, not u), and the truncation moves by the integer 17 P.  So over a key
// interval whose holders in EVERY launch lie in such regions, launch j holds key t exactly when it holds t + 17 P, as often,
// and the mask of (k, g) equals that of (k, g + P).
// The events that end a region, as keys: a_i of launch j leaves a binade at 2^b where key - a_i = s_j + (the lamp terms
// still to come) + rounding, that is within L + E of 2^b + s_j, and a4 within 1 of 2^b, with L = ceil(13|lx| + 7|ly| + 11|lz|)
// and E = 32 >= five roundings of at most half an ulp of 8 (keys below 2^27) plus the truncation; a launch's first and last key
// of the call's range (beyond them it holds nothing); and the key of work-item 0, which reads the other SEED.  Below
// FLOOR = max s_j + L + E + 1 a sum may not be positive, and from 2^27 on a launch may hold a key twice: no interiors there.
// These are dedupe_class_tally's cuts, taken for EVERY binade (a fractional lamp term rounds differently in each binade below
// 2^24, which a tally may ignore and a table may not) plus work-item 0's key.
// The margin.  An occurrence with key t looks at key t in every launch, never at another key, so nothing of the offsets
// between launches enters: an interior is a stratum shrunk at both ends by M = L + E + 34 DEDUPE_PERIOD_MAX keys -- L + E
// for where an event really lies, and two periods of 17 P keys so that g - P and g + P of every holder stay inside.
// The proof is never trusted alone: the table is built from one tile at each end of the interior with the tile functions of
// the mark pass, every gid of both tiles must agree with its residue's entry, and a stratum that fails, or that shows a key
// held twice, goes back to the general path.  So do gid 0, groups of more than DEDUPE_PERIODIC_LAUNCHES launches, interiors
// shorter than four of the widest build tiles, and whatever does not fit the caps: the DEDUPE_PERIODIC_STRATA longest interiors are taken
// while their K P words fit DEDUPE_PERIODIC_WORDS (the headline's group: 12 interiors and 256 words hold 0.975 of its
// occurrences, the nine long ones 0.97; a route's group of 5 launches takes fewer words).
constexpr int DEDUPE_PERIODIC_STRATA = 12;
constexpr int DEDUPE_PERIODIC_WORDS = 384;
constexpr int DEDUPE_PERIOD_MAX = 16;           // gids: 2 ulp with ulp <= 8 below 2^27
constexpr int DEDUPE_PERIODIC_LAUNCHES = 30;
constexpr bool DEDUPE_PERIODIC_DEFAULT = true;  // uvrt_set_dedupe_periodic's default (DESIGN.md section 15 has the measurement)
constexpr int32_t DEDUPE_PERIODIC_TILE = 68 * DEDUPE_PERIOD_MAX;   // keys of the widest build tile: 68 P, four periods of every launch's gids

struct DedupePeriodic {
    int32_t count;                                  // interiors, ascending in the key; 0: everything takes the general path
    int32_t key_lo[DEDUPE_PERIODIC_STRATA];         // interior s holds the keys [key_lo, key_lo + keys)
    uint32_t keys[DEDUPE_PERIODIC_STRATA];
    int32_t period[DEDUPE_PERIODIC_STRATA];         // gids, a power of two
    int32_t word_off[DEDUPE_PERIODIC_STRATA];       // words[word_off + k * period + (gid & (period - 1))]
    // the deposit word of the occurrence (dedupe_deposit_word), 0 = absorbed; room behind the last word for a reader that
    // takes DEDUPE_PERIOD_MAX words wherever a launch's P words start
    uint32_t words[DEDUPE_PERIODIC_WORDS + DEDUPE_PERIOD_MAX];
};

// the interior that holds `key`, or -1
UVRT_HD int dedupe_periodic_find(const DedupePeriodic& T, int32_t key)
{
    for (int s = 0; s < T.count; ++s)
        if ((uint32_t)key - (uint32_t)T.key_lo[s] < T.keys[s]) return s;
    return -1;
}
UVRT_HD int32_t dedupe_periodic_index(const DedupePeriodic& T, int s, int k, int32_t gid)
{
    return T.word_off[s] + k * T.period[s] + (gid & (T.period[s] - 1));
}
// the owners among launch k's gids [x0, x1) (x0 >= 1, inside the call's range) that lie in an interior; `words`: T.words or a copy
UVRT_HD uint32_t dedupe_periodic_owners(const DedupeGroup& G, const DedupePeriodic& T, const uint32_t* words, int k, int32_t x0, int32_t x1)
{
    if (x0 >= x1) return 0u;
    const uint32_t seed1 = dedupe_seed1(G, k);
    const int32_t ka = dedupe_key1_of(G, seed1, x0), kb = dedupe_key1_of(G, seed1, x1 - 1);
    uint32_t total = 0u;
    for (int s = 0; s < T.count; ++s) {
        const int64_t A = T.key_lo[s], B = A + (int64_t)T.keys[s];
        if ((int64_t)kb < A || (int64_t)ka >= B) continue;
        const int32_t a = (int64_t)ka >= A ? x0 : dedupe_lower_bound(G, k, A, x0, x1);
        const int32_t b = (int64_t)kb < B ? x1 : dedupe_lower_bound(G, k, B, a, x1);
        // residue (a + r) mod P comes q times among [a, b), and once more for r below the rest
        const int32_t P = T.period[s], n = b - a, q = n / P, rest = n & (P - 1);
        for (int32_t r = 0; r < P; ++r)
            if (words[dedupe_periodic_index(T, s, k, a + r)] != 0u) total += (uint32_t)(q + (r < rest));
    }
    return total;
}

// What the mark pass walks of a chunk's keys [key_lo, key_lo + keys): the intervals between the interiors, each in strips of
// `strip` tiles of W keys.  gap_key / gap_keys: room for DEDUPE_PERIODIC_STRATA + 1; strip0: one more, the running strip
// count (strip0[gaps] = the strips of all).  Returns the gaps.
inline int dedupe_periodic_gaps(const DedupePeriodic& T, int64_t key_lo, int64_t keys, int32_t W, int32_t strip, int32_t* gap_key,
                                uint32_t* gap_keys, int32_t* strip0)
{
    int n = 0;
    int64_t cur = key_lo, strips = 0;
    const int64_t end = key_lo + keys;
    const auto gap = [&](int64_t a, int64_t b) {
        gap_key[n] = (int32_t)a;
        gap_keys[n] = (uint32_t)(b - a);
        strip0[n++] = (int32_t)strips;
        strips += ((b - a + W - 1) / W + strip - 1) / strip;
    };
    for (int s = 0; s < T.count && cur < end; ++s) {
        const int64_t A = T.key_lo[s], B = A + (int64_t)T.keys[s];
        if (B <= cur || A >= end) continue;
        if (A > cur) gap(cur, A);
        cur = B;
    }
    if (cur < end) gap(cur, end);
    strip0[n] = (int32_t)strips;
    return n;
}

// Host: one build tile of an interior with period P, the keys [t0, t0 + 68 P): the mask of every residue of every launch
// into out[k * P + r].  false: a key held twice, a residue without a gid, or two gids of one residue that differ.
inline bool dedupe_periodic_tile(const DedupeGroup& G, int64_t t0, int32_t P, uint32_t* table, uint32_t* out)
{
    const int32_t W = 68 * P;
    int32_t g_lo[DEDUPE_MAX], g_hi[DEDUPE_MAX];
    if (dedupe_tile_fill(G, t0, W, nullptr, table, g_lo, g_hi)) return false;
    for (int32_t i = 0; i < W; ++i)
        if (table[i] & DEDUPE_MANY) return false;
    for (int k = 0; k < G.count; ++k) {
        if (g_hi[k] - g_lo[k] < P) return false;
        for (int32_t g = g_lo[k]; g < g_hi[k]; ++g) {
            const uint32_t mask = dedupe_tile_resolve(table[dedupe_tile_slot(dedupe_key1(G, k, g), t0)], k);
            uint32_t& e = out[k * P + (g & (P - 1))];
            if (g - g_lo[k] < P) e = mask;
            else if (e != mask) return false;
        }
    }
    return true;
}

// Host: the group's interiors and their tables (the words through the group's class table C, as k_dedupe_write translates a
// mask; C.count 0: the masks themselves).  `table`: DEDUPE_TILE_KEYS entries.  A function of the group and C alone.
inline void dedupe_periodic_build(const DedupeGroup& G, const DedupeClasses& C, uint32_t* table, DedupePeriodic& T)
{
    static_assert(DEDUPE_PERIODIC_TILE <= DEDUPE_TILE_KEYS, "the build tile fits the host's table");
    T = DedupePeriodic{};
    const int K = G.count;
    const int64_t last = G.first_gid + G.n - 1, lo1 = G.first_gid > 1 ? G.first_gid : 1;
    if (K > DEDUPE_PERIODIC_LAUNCHES || lo1 > last) return;
    const double lamp = 13.0 * (double)(G.lx < 0 ? -G.lx : G.lx) + 7.0 * (double)(G.ly < 0 ? -G.ly : G.ly) + 11.0 * (double)(G.lz < 0 ? -G.lz : G.lz);
    if (!(lamp < 1e6)) return;
    const int64_t L = (int64_t)lamp + 1, E = 32, M = L + E + 34 * DEDUPE_PERIOD_MAX;
    constexpr int BINADES = 27;                   // 2^0 .. 2^26; the keys from 2^27 on are left out below
    int64_t cut[3 * DEDUPE_MAX + BINADES * (DEDUPE_MAX + 1) + 2];
    int64_t klo, khi, smax = 0;
    dedupe_key_span(G, lo1, last, klo, khi);
    for (int j = 0; j < K; ++j) smax = std::max(smax, (int64_t)(dedupe_seed1(G, j) >> 15));
    const int64_t floor_key = smax + L + E + 1;
    klo = klo < floor_key ? floor_key : klo;
    khi = khi > ((int64_t)1 << 27) ? ((int64_t)1 << 27) : khi;
    if (khi - klo < 2 * M) return;
    const int ncut = dedupe_cuts(G, lo1, last, 0, BINADES - 1, true, klo, khi, cut);
    // the candidates: every stratum's interior that is long enough, then the longest that fit the caps
    struct Cand { int64_t a, b; int32_t P; };
    Cand cand[DEDUPE_PERIODIC_STRATA + 1];
    int nc = 0, words = 0;
    for (int i = 0; i + 1 < ncut; ++i) {
        const int64_t a = (cut[i] < klo ? klo : cut[i]) + M, b = (cut[i + 1] > khi ? khi : cut[i + 1]) - M;
        if (b - a < 4 * (int64_t)DEDUPE_PERIODIC_TILE) continue;
        int64_t ulp = 1;
        while (((int64_t)1 << 24) * ulp < b + M) ulp += ulp;      // (b + M: the stratum's last key; no power of two inside it)
        const Cand v = {a, b, (int32_t)(2 * ulp)};
        if (v.P > DEDUPE_PERIOD_MAX) continue;
        int at = nc;                              // by length, longest first; the list keeps one more than the cap and drops the last
        for (; at > 0 && cand[at - 1].b - cand[at - 1].a < b - a; --at) cand[at] = cand[at - 1];
        cand[at] = v;
        if (nc < DEDUPE_PERIODIC_STRATA) ++nc;
    }
    int take = 0;
    for (; take < nc && words + K * cand[take].P <= DEDUPE_PERIODIC_WORDS; ++take) words += K * cand[take].P;
    for (int i = 1; i < take; ++i) {              // back into key order
        const Cand v = cand[i];
        int at = i;
        for (; at > 0 && cand[at - 1].a > v.a; --at) cand[at] = cand[at - 1];
        cand[at] = v;
    }
    uint32_t first[DEDUPE_PERIODIC_LAUNCHES * DEDUPE_PERIOD_MAX], second[DEDUPE_PERIODIC_LAUNCHES * DEDUPE_PERIOD_MAX];
    int32_t off = 0;
    for (int i = 0; i < take; ++i) {
        const Cand& v = cand[i];
        const int32_t P = v.P;
        // a tile at each end (a residue is the gid's own, gid mod P: the two tiles compare like with like)
        if (!dedupe_periodic_tile(G, v.a, P, table, first) || !dedupe_periodic_tile(G, v.b - 68 * P, P, table, second)) continue;
        bool same = true;
        for (int e = 0; e < K * P; ++e) same = same && first[e] == second[e];
        if (!same) continue;
        const int s = T.count++;
        T.key_lo[s] = (int32_t)v.a;
        T.keys[s] = (uint32_t)(v.b - v.a);
        T.period[s] = P;
        T.word_off[s] = off;
        for (int e = 0; e < K * P; ++e)
            T.words[off + e] = first[e] == 0u ? 0u : dedupe_deposit_word(C.count > 0, C.slot_mask, C.slot_word, first[e]);
        off += K * P;
    }
}

// Host: the masks of the chunk [c0, c0 + cn) as a chunk's generate finds them with the table T (built WITHOUT classes: its
// words are the masks) -- the gaps tile by tile, the interiors from the table -- and the owners per launch and block of
// `block` gids, counts[k * ceil(cn / block) + b], the interiors' in closed form.  Returns the occurrences taken from the table.
inline int64_t dedupe_plan_periodic(const DedupeGroup& G, const DedupePeriodic& T, int32_t W, int32_t strip, int32_t block, int64_t c0,
                                    int64_t cn, uint32_t* table, uint32_t* masks, uint32_t* counts)
{
    const int64_t nb = (cn + block - 1) / block;
    for (int64_t i = 0; i < (int64_t)G.count * cn; ++i) masks[i] = 0u;
    int64_t key_lo, tiles;
    dedupe_tile_range(G, c0, cn, W, key_lo, tiles);
    int32_t gap_key[DEDUPE_PERIODIC_STRATA + 1], strip0[DEDUPE_PERIODIC_STRATA + 2];
    uint32_t gap_keys[DEDUPE_PERIODIC_STRATA + 1];
    const int gaps = dedupe_periodic_gaps(T, key_lo, tiles * W, W, strip, gap_key, gap_keys, strip0);
    for (int i = 0; i < gaps; ++i) dedupe_plan_tiled_keys(G, W, strip, c0, cn, gap_key[i], gap_keys[i], table, masks);
    int64_t from_table = 0;
    for (int k = 0; k < G.count; ++k) {
        for (int64_t b = 0; b < nb; ++b) {
            const int64_t x0 = c0 + b * block, x1 = x0 + block < c0 + cn ? x0 + block : c0 + cn;
            uint32_t owners = 0u;
            for (int64_t g = x0; g < x1; ++g) owners += masks[(int64_t)k * cn + (g - c0)] != 0u;      // (the gaps' only, so far)
            counts[(int64_t)k * nb + b] = owners + dedupe_periodic_owners(G, T, T.words, k, (int32_t)(x0 > 1 ? x0 : 1), (int32_t)x1);
        }
        for (int64_t g = c0 > 1 ? c0 : 1; g < c0 + cn; ++g) {
            const int s = dedupe_periodic_find(T, dedupe_key1(G, k, (int32_t)g));
            if (s < 0) continue;
            masks[(int64_t)k * cn + (g - c0)] = T.words[dedupe_periodic_index(T, s, k, (int32_t)g)];
            ++from_table;
        }
    }
    return from_table;
}

}  // namespace uvrt

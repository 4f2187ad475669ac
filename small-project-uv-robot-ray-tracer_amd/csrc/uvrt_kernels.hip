// uvrt_kernels.hip -- hand-written CDNA4 (gfx950) kernels of the UV-dose hot path.
//
// Compile with -ffp-contract=off and correctly rounded f32 divide/sqrt (csrc/Makefile): every
// result must equal the reference kernels' strict-IEEE arithmetic bit for bit, so each
// operator below is one rounding in the order the reference source writes it.
//
//   k_generate        cl/generate.cl:8-40       + optional coherence key / rank, extend's per-launch records
//   k_scan_bins, k_scatter                      optional counting sort of rays by coherence key
//   (k_extend6        cl/extend.cl:6-99         BVH traversal + photon deposit, THE hot loop: uvrt_extend6.hip)
//   k_accumulate      cl/accumulate.cl:4-14
//   k_reset           cl/reset.cl:4-26
//   k_compute_dosage  cl/shade.cl:23-41
//   k_dosage_to_color cl/shade.cl:4-21,43-71
#include "uvrt_device.h"

namespace uvrt {

// --------------------------------------------------------------- generate, cl/generate.cl

// Spread the quantised (azimuth, elevation, height) of a photon over one key so that rays
// close in the key are close in space; most-significant bits first, round-robin over the
// three coordinates.  Only the ORDER in which rays are traced depends on it.
__device__ __forceinline__ uint32_t coherence_key(uint32_t qphi, uint32_t qy, uint32_t qo,
                                                  int bphi, int by, int bo)
{
    uint32_t key = 0;
    while (bphi > 0 || by > 0 || bo > 0) {
        if (bphi > 0) { --bphi; key = (key << 1) | ((qphi >> bphi) & 1u); }
        if (by > 0) { --by; key = (key << 1) | ((qy >> by) & 1u); }
        if (bo > 0) { --bo; key = (key << 1) | ((qo >> bo) & 1u); }
    }
    return key;
}

__global__ __launch_bounds__(256) void k_generate(GenParams p)
{
    helper_priority(p.prio);
    if (blockIdx.x >= p.ray_blocks) {   // extra workgroups: extend v6's per-launch node-pair records
        const int j = (int)(blockIdx.x - p.ray_blocks) * 256 + threadIdx.x;
        if (j < p.prep_npairs) prepare_record6(p.prep_pairs, p.prep_recs, p.lx, p.lz, p.prep_npairs, j, p.prep_perm);
        return;
    }
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int64_t gid = p.first_gid + i;
    float r0;
    double x, y;
    const float4 ray = generate_ray(p.lx, p.ly, p.lz, p.light_length, gid, p.seed_prev, p.seed_next, p.seed_mode, r0, x, y);
    const float diry = ray.y;
    p.rays[i] = ray;                                                      // :31-37

    if (p.keyrank) {
        // azimuth as a diamond angle in [0,4): monotone in the true angle, one division
        const float fx = (float)x, fy = (float)y;
        const float ax = fabsf(fx), ay = fabsf(fy);
        float t = ay / (ax + ay + 1e-30f);
        float ang = fx >= 0.0f ? (fy >= 0.0f ? t : 4.0f - t) : (fy >= 0.0f ? 2.0f - t : 2.0f + t);
        const uint32_t nphi = 1u << p.bits_phi, ny = 1u << p.bits_y, no = 1u << p.bits_o;
        uint32_t qphi = min((uint32_t)(ang * (0.25f * (float)nphi)), nphi - 1);
        uint32_t qy = min((uint32_t)((diry + 1.0f) * (0.5f * (float)ny)), ny - 1);
        uint32_t qo = min((uint32_t)(r0 * (float)no), no - 1);
        const uint32_t key = coherence_key(qphi, qy, qo, p.bits_phi, p.bits_y, p.bits_o);
        const uint32_t rank = atomicAdd(&p.hist[key], 1u);
        p.keyrank[i] = make_uint2(key, rank);
    }
}

// The rays of several launches side by side (uvrt_trace_batch): blockIdx.y = physical plane, every plane
// generates the same global-id range under its own lamp and place in the SEED chain.
__global__ __launch_bounds__(256) void k_generate_batch(GenBatchParams p)
{
    helper_priority(p.prio);
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= p.n) return;
    const int k = blockIdx.y;
    float r0;
    double x, y;
    p.rays[(int64_t)k * p.n_pad + i] = generate_ray(p.lx[k], p.ly[k], p.lz[k], p.light_length, p.first_gid + i,
                                                    p.seed_prev[k], p.seed_next[k], p.seed_mode, r0, x, y);
}

// The distinct rays of a dedupe group (GenDedupeParams).  Scan and write: blockIdx.y = launch of the group, blockIdx.x =
// DD_SLOTS gids of the chunk, DD_ROUNDS per thread (few workgroup counts for the one-workgroup scan between the passes).
//
// mark: every occurrence's mask (uvrt_dedupe.h: 0 = another occurrence traces this ray) and the owners per launch and block
// of DD_SLOTS gids.  One WAVE per strip of key tiles (uvrt_dedupe.h, "strips of narrow tiles"), a workgroup of its own: beside
// the other lane's persistent traversal grid a CU has four wave slots and 20 KB of LDS left, and four such workgroups of
// 3 840 B take them and cover each other's waits; none waits for another.  Per tile every launch's gid run goes into a table
// in LDS with one OR each and nothing read back -- the run's end is where its keys leave the tile, and that is the next
// tile's start -- then every occurrence of the chunk reads its mask from its key's entry.  The owners are counted with
// integer adds: a ballot per round, kept by lane j for launch j while the strip stays in one block, one global add per block
// and strip -- so the counts and the compaction order stay a function of the group alone.  block_counts is zero on entry
// (k_dedupe_write leaves it so).
__global__ __launch_bounds__(64) void k_dedupe_mark(GenDedupeParams p)
{
    helper_priority(p.prio);
    constexpr int32_t W = DEDUPE_MARK_KEYS;
    __shared__ uint32_t s_table[W];
    const int lane = threadIdx.x, K = p.g.count;
    const uint32_t nb = (uint32_t)((p.gn + DD_SLOTS - 1) / DD_SLOTS);
    // (gids as int32: the range ends below DEDUPE_GID_END)
    const int32_t lo = (int32_t)(p.g.first_gid > 1 ? p.g.first_gid : 1), hi = (int32_t)(p.g.first_gid + p.g.n);
    const int32_t c0 = (int32_t)p.g0, c1 = (int32_t)(p.g0 + p.gn);
    if ((int32_t)blockIdx.x >= p.gap_strip0[p.gaps]) {
        // extra workgroups: the owners of the interiors of the period table, a thread per launch and block of DD_SLOTS gids, in
        // closed form from the table (neither tmp nor the key table see those occurrences)
        // (the words once into LDS: the arguments are quick to read for scalar loads only)
        static_assert(DEDUPE_PERIODIC_WORDS % 64 == 0 && DEDUPE_PERIODIC_WORDS <= W, "the words fit the key table's LDS in whole rounds");
#pragma unroll
        for (int i = 0; i < DEDUPE_PERIODIC_WORDS; i += 64) s_table[i + lane] = p.per.words[i + lane];
        __syncthreads();
        const uint32_t t = (blockIdx.x - (uint32_t)p.gap_strip0[p.gaps]) * 64u + (uint32_t)lane;
        if (t < (uint32_t)K * nb) {
            const uint32_t k = t / nb, b = t - k * nb;
            const int32_t x0 = c0 + (int32_t)(b * (uint32_t)DD_SLOTS), x1 = min(x0 + DD_SLOTS, c1);
            const uint32_t owners = dedupe_periodic_owners(p.g, p.per, s_table, (int)k, max(x0, 1), x1);
            if (owners != 0u) atomicAdd(&p.block_counts[t], owners);
        }
        return;
    }
    // the workgroup's strip: of the key interval `gap` (uniform: scalar loads and compares)
    int gap = 0;
    while (gap + 1 < p.gaps && (int32_t)blockIdx.x >= p.gap_strip0[gap + 1]) ++gap;
    const int64_t gap_lo = p.gap_key[gap];
    const uint32_t gap_keys = p.gap_keys[gap];
    const int64_t gap_tiles = (int64_t)((gap_keys + (uint32_t)W - 1u) / (uint32_t)W);
    const int64_t tile0 = (int64_t)((int32_t)blockIdx.x - p.gap_strip0[gap]) * p.strip_tiles;
    const int64_t tile1 = tile0 + p.strip_tiles < gap_tiles ? tile0 + p.strip_tiles : gap_tiles;
    // lane j keeps what is uniform per launch j: its run [run_lo, run_hi) in the current tile, and the owners of its current
    // block that no global add has taken yet; its SEED and the key of its gid 0, so that no loop below waits for a load
    int32_t run_lo = hi, run_hi = hi, key0 = 0;
    uint32_t seed1 = 0u;
    if (lane < K) {
        run_lo = dedupe_strip_first(p.g, lane, gap_lo + tile0 * W);      // the strip's one search per launch
        seed1 = dedupe_seed1(p.g, lane);
        key0 = p.g.key0[lane];
    }
    uint32_t cnt_block = 0u, cnt = 0u;
    const auto add_owners = [&](int j, uint32_t block, uint32_t owners) { atomicAdd(&p.block_counts[(size_t)j * nb + block], owners); };
    const auto count_owners = [&](int j, uint32_t block, uint32_t owners) {        // (uniform arguments)
        if (lane == j && owners != 0u) {
            if (block != cnt_block) {
                if (cnt != 0u) add_owners(j, cnt_block, cnt);
                cnt_block = block;
                cnt = 0u;
            }
            cnt += owners;
        }
    };
    for (int64_t tile = tile0; tile < tile1; ++tile) {
        const int64_t t0 = gap_lo + tile * W;
        const int32_t w = (int32_t)min((uint32_t)W, gap_keys - (uint32_t)(tile * W));      // (the interval's last tile ends with it)
        static_assert(W % 64 == 0, "the wave zeroes the table in whole rounds");
#pragma unroll
        for (int i = 0; i < W; i += 64) s_table[i + lane] = 0u;
        __syncthreads();      // (a workgroup of one wave: no s_barrier, the wave's LDS accesses stay in order)
        // insert: launch j's run from its g_lo on, 64 gids a round, until its keys leave the tile -- that is its g_hi
        for (int j = 0; j < K; ++j) {
            int32_t base = __builtin_amdgcn_readlane(run_lo, j);
            const uint32_t seed = (uint32_t)__builtin_amdgcn_readlane((int)seed1, j);
            for (;;) {
                const int32_t g = base + lane;
                bool in = false;
                if (g < hi) {
                    const int32_t key = dedupe_key1_of(p.g, seed, g);
                    in = dedupe_in_tile(key, t0, w);
                    if (in) dedupe_tile_insert_run(s_table, dedupe_tile_slot(key, t0), j, dedupe_run_twice(p.g, seed, g, key, lo, hi));
                }
                const int32_t n_in = (int32_t)__popcll(__builtin_amdgcn_ballot_w64(in));      // (a prefix of the lanes: the keys never decrease)
                base += n_in;
                if (n_in < 64) break;
            }
            if (lane == j) run_hi = base;
        }
        const bool holds0 = lane < K && dedupe_tile_holds_key0(p.g, key0, t0, w);      // gid 0 of launch `lane`: last, reading the entry
        if (holds0) dedupe_tile_insert(s_table, dedupe_tile_slot(key0, t0), lane);
        __syncthreads();
        // resolve: every occurrence of the chunk reads its mask from its key's entry; the owners per block of DD_SLOTS gids
        for (int j = 0; j < K; ++j) {
            const int32_t a = max(__builtin_amdgcn_readlane(run_lo, j), c0), b = min(__builtin_amdgcn_readlane(run_hi, j), c1);
            const uint32_t seed = (uint32_t)__builtin_amdgcn_readlane((int)seed1, j);
            for (int32_t base = a; base < b; base += 64) {                    // (uniform trips: every lane takes part in the ballots)
                const int32_t g = base + lane;
                const uint32_t fb = (uint32_t)(base - c0) / (uint32_t)DD_SLOTS;      // the round's first block; 64 gids touch two at most
                uint32_t mask = 0u, blk = fb;
                if (g < b) {
                    const uint32_t slot = dedupe_tile_slot(dedupe_key1_of(p.g, seed, g), t0);
                    mask = dedupe_tile_resolve(slot < (uint32_t)w ? s_table[slot] : DEDUPE_MANY, j);
                    p.tmp[(int64_t)j * p.gn + (g - c0)] = mask;
                    blk = (uint32_t)(g - c0) / (uint32_t)DD_SLOTS;
                }
                const int32_t last = min(base + 63, b - 1);
                if ((uint32_t)(last - c0) / (uint32_t)DD_SLOTS == fb) {      // (uniform; one round in 32 meets a block's end)
                    count_owners(j, fb, (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(mask != 0u)));
                } else {
                    const uint32_t n0 = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(mask != 0u && blk == fb));
                    const uint32_t n1 = (uint32_t)__popcll(__builtin_amdgcn_ballot_w64(mask != 0u && blk != fb));
                    count_owners(j, fb, n0);
                    count_owners(j, fb + 1u, n1);
                }
            }
        }
        if (c0 == 0 && holds0) {      // work-item 0 of launch `lane`
            const uint32_t mask = dedupe_tile_resolve(s_table[dedupe_tile_slot(key0, t0)], lane);
            p.tmp[(int64_t)lane * p.gn] = mask;
            if (mask != 0u) add_owners(lane, 0u, 1u);
        }
        run_lo = run_hi;      // carried: where a launch's keys left this tile they enter the next
        __syncthreads();      // (the table is zeroed again behind the reads)
    }
    if (lane < K && cnt != 0u) add_owners(lane, cnt_block, cnt);
}

// scan: the workgroups' counts -> their first slot in the compacted list, in (launch, gid) order; the total.  One workgroup
// of 256 threads: it must find room on a CU beside the persistent traversal grid of the other lane, as every kernel here.
__global__ __launch_bounds__(256) void k_dedupe_scan(uint32_t* block_counts, uint32_t* total, uint32_t* deposits, uint32_t nblocks, int prio)
{
    helper_priority(prio);
    __shared__ uint32_t s_part[256];
    const uint32_t tid = threadIdx.x;
    if (tid == 0u) *deposits = 0u;      // (the write pass adds to it, one add per workgroup)
    const uint32_t per = (nblocks + 255u) / 256u;
    const uint32_t lo = min(tid * per, nblocks), hi = min(lo + per, nblocks);
    uint32_t sum = 0;
    for (uint32_t b = lo; b < hi; ++b) sum += block_counts[b];
    s_part[tid] = sum;
    __syncthreads();
    for (uint32_t off = 1; off < 256u; off <<= 1) {
        const uint32_t v = tid >= off ? s_part[tid - off] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (uint32_t b = lo; b < hi; ++b) {
        const uint32_t c = block_counts[b];
        block_counts[b] = run;
        run += c;
    }
    if (tid == 255u) *total = s_part[255];
}

// write: the owners' rays (generate.cl:11-37) and deposit words at their slots, in (launch, gid) order.  The word is the mask
// translated through the group's class table (uvrt_dedupe.h "mask classes"; the table comes with the parameters and is
// looked up in LDS); the atomics the words stand for are counted, one add per workgroup.
__global__ __launch_bounds__(256) void k_dedupe_write(GenDedupeParams p)
{
    helper_priority(p.prio);
    __shared__ uint32_t s_cnt[DD_ROUNDS][4];
    __shared__ uint32_t s_slot_mask[DEDUPE_CLASS_SLOTS], s_slot_word[DEDUPE_CLASS_SLOTS], s_dep;
    if (threadIdx.x < (unsigned)DEDUPE_CLASS_SLOTS) {
        s_slot_mask[threadIdx.x] = p.cls.slot_mask[threadIdx.x];
        s_slot_word[threadIdx.x] = p.cls.slot_word[threadIdx.x];
    }
    if (threadIdx.x == 0) s_dep = 0u;
    const bool classes = p.cls.count > 0;
    uint32_t dep = 0u;
    const int k = blockIdx.y;
    const uint32_t wv = threadIdx.x >> 6;
    // The period table (uvrt_dedupe.h): which interiors hold keys of this workgroup's gids, from the keys at its ends -- uniform,
    // every interior's bounds in one round of scalar loads; `inside`: one interior holds them all, so a gid needs no key.  An
    // occurrence of an interior takes its WORD from the table (mark wrote nothing for it), every other one its mask from tmp;
    // `worded` says which, a bit per round.  The table travels in the kernel's arguments, which only scalar loads read
    // quickly: a period divides 256, so a thread's gids of all rounds share one residue, and its word of an interior is
    // picked from the interior's DEDUPE_PERIOD_MAX scalar words once per workgroup -- no vector load, no LDS, no barrier (a
    // workgroup beside a traversal is alone on its CU and lives by its waits).
    static_assert(256 % DEDUPE_PERIOD_MAX == 0, "a thread's rounds share their residue");
    uint32_t near = 0u, worded = 0u;
    bool inside = false;
    const uint32_t seed1 = dedupe_seed1(p.g, k);
    const int32_t gid0 = (int32_t)(p.g0 + (int64_t)blockIdx.x * DD_SLOTS) + (int32_t)threadIdx.x;      // the thread's gid of round 0
    if (p.per.count > 0) {
        const int32_t x0 = max((int32_t)(p.g0 + (int64_t)blockIdx.x * DD_SLOTS), 1);
        const int32_t x1 = (int32_t)min(p.g0 + ((int64_t)blockIdx.x + 1) * DD_SLOTS, p.g0 + p.gn);
        const int32_t ka = __builtin_amdgcn_readfirstlane(dedupe_key1_of(p.g, seed1, x0));
        const int32_t kb = __builtin_amdgcn_readfirstlane(dedupe_key1_of(p.g, seed1, x1 - 1));
#pragma unroll
        for (int s = 0; s < DEDUPE_PERIODIC_STRATA; ++s) {      // (keys below 2^27: the bounds are int32)
            const int32_t A = p.per.key_lo[s], B = A + (int32_t)p.per.keys[s];
            if (s < p.per.count && kb >= A && ka < B) {
                near |= 1u << s;
                inside = ka >= A && kb < B;
            }
        }
    }
    uint32_t mask[DD_ROUNDS], rank[DD_ROUNDS];
#pragma unroll
    for (int r = 0; r < DD_ROUNDS; ++r) mask[r] = 0u;
    for (uint32_t left = near; left != 0u; left &= left - 1u) {      // (uniform: one interior, two or three at a cluster of events)
        const int s = __builtin_ctz(left);
        const int32_t A = p.per.key_lo[s], P = p.per.period[s];
        const uint32_t len = p.per.keys[s];
        const uint32_t* w = &p.per.words[p.per.word_off[s] + k * P];
        const int32_t res = gid0 & (P - 1);
        uint32_t word = 0u;
#pragma unroll
        for (int q = 0; q < DEDUPE_PERIOD_MAX; ++q) {          // (words[] has room for the reads past the launch's P words)
            const uint32_t wq = w[q];
            if (res == q) word = wq;
        }
#pragma unroll
        for (int r = 0; r < DD_ROUNDS; ++r) {
            const int64_t i = (int64_t)blockIdx.x * DD_SLOTS + r * 256 + threadIdx.x;
            const int32_t g = gid0 + r * 256;
            if (i < p.gn && g >= 1 && (inside || (uint32_t)dedupe_key1_of(p.g, seed1, g) - (uint32_t)A < len)) {
                mask[r] = word;
                worded |= 1u << r;
            }
        }
    }
    uint32_t pos = p.block_counts[(size_t)k * gridDim.x + blockIdx.x];      // (after the scan: the workgroup's first slot)
#pragma unroll
    for (int r = 0; r < DD_ROUNDS; ++r) {
        const int64_t i = (int64_t)blockIdx.x * DD_SLOTS + r * 256 + threadIdx.x;
        if (!((worded >> r) & 1u) && i < p.gn) mask[r] = p.tmp[(int64_t)k * p.gn + i];
        const unsigned long long owners = __builtin_amdgcn_ballot_w64(mask[r] != 0u);
        rank[r] = __builtin_amdgcn_mbcnt_hi((uint32_t)(owners >> 32), __builtin_amdgcn_mbcnt_lo((uint32_t)owners, 0u));
        if ((threadIdx.x & 63u) == 0u) s_cnt[r][wv] = (uint32_t)__popcll(owners);
    }
    __syncthreads();
    // every thread has read the entry: zero again for the next chunk's mark, which adds its owners to it
    if (threadIdx.x == 0) p.block_counts[(size_t)k * gridDim.x + blockIdx.x] = 0u;
#pragma unroll
    for (int r = 0; r < DD_ROUNDS; ++r) {
        for (uint32_t w = 0; w < 4u; ++w) {
            if (w == wv && mask[r] != 0u) {
                const int64_t i = (int64_t)blockIdx.x * DD_SLOTS + r * 256 + threadIdx.x;
                float r0;
                double x, y;
                p.rays[pos + rank[r]] = generate_ray(p.g.lx, p.g.ly, p.g.lz, p.light_length, p.g0 + i, p.g.seed_prev[k],
                                                     p.g.seed_next[k], p.g.seed_mode, r0, x, y);
                const uint32_t word = ((worded >> r) & 1u) ? mask[r] : dedupe_deposit_word(classes, s_slot_mask, s_slot_word, mask[r]);
                p.masks[pos + rank[r]] = word;
                dep += (uint32_t)dedupe_word_deposits(classes, word);
            }
            pos += s_cnt[r][w];
        }
    }
    if (dep != 0u) atomicAdd(&s_dep, dep);
    __syncthreads();
    if (threadIdx.x == 0 && s_dep != 0u) atomicAdd(p.deposits, s_dep);
}

// Exclusive prefix sum over the key histogram (one 1024-thread workgroup; nbins <= 2^20), and
// re-zero the histogram for the next launch.
__global__ __launch_bounds__(1024) void k_scan_bins(uint32_t* hist, uint32_t* bin_start,
                                                    int32_t nbins)
{
    __shared__ uint32_t s_part[1024];
    const int tid = threadIdx.x;
    const int per = (nbins + 1023) / 1024;
    const int lo = tid * per, hi = min(lo + per, nbins);
    uint32_t sum = 0;
    for (int b = lo; b < hi; ++b) sum += hist[b];
    s_part[tid] = sum;
    __syncthreads();
    for (int off = 1; off < 1024; off <<= 1) {
        uint32_t v = tid >= off ? s_part[tid - off] : 0u;
        __syncthreads();
        s_part[tid] += v;
        __syncthreads();
    }
    uint32_t run = s_part[tid] - sum;
    for (int b = lo; b < hi; ++b) {
        const uint32_t c = hist[b];
        bin_start[b] = run;
        hist[b] = 0;
        run += c;
    }
}

__global__ __launch_bounds__(256) void k_scatter(const float4* __restrict__ rays,
                                                 const uint2* __restrict__ keyrank,
                                                 const uint32_t* __restrict__ bin_start,
                                                 float4* __restrict__ sorted,
                                                 uint32_t* __restrict__ order, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= n) return;
    const uint2 kr = keyrank[i];
    const uint32_t pos = bin_start[kr.x] + kr.y;
    const float4 r = rays[i];
    sorted[pos] = r;
    order[pos] = (uint32_t)i;
}

// ----------------------------------------------------------- per-triangle kernels (O(T))

// accumulate.cl:4-14; tempPhotonMap[i] is the (exact, integer) sum of the deposit replicas.
// Four lanes share a triangle: each sums (and clears) a quarter of the replicas, two DPP adds
// combine them, lane 0 of the quad applies the reference's update.
__global__ __launch_bounds__(256) void k_accumulate(double* __restrict__ photon_map,
                                                    double* __restrict__ max_map,
                                                    int32_t* __restrict__ counts, int32_t replicas,
                                                    int64_t stride, float time_step, int32_t T, int prio)
{
    helper_priority(prio);
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int i = g >> 2, part = g & 3;
    int32_t total = 0;
    if (i < T) {
        for (int r = part; r < replicas; r += 4) {
            total += counts[r * stride + i];
            counts[r * stride + i] = 0;
        }
    }
    total += __builtin_amdgcn_mov_dpp(total, 0xb1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    total += __builtin_amdgcn_mov_dpp(total, 0x4e, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    if (i >= T || part != 0) return;
    const double c = (double)total;
    photon_map[i] = photon_map[i] + c * (double)time_step;
    const double m = max_map[i];
    max_map[i] = m < c ? c : m;
}

// tempPhotonMap in the reference's single-array form: replica 0 = sum, the others zero
__global__ __launch_bounds__(256) void k_fold_counts(int32_t* __restrict__ counts, int32_t replicas,
                                                     int64_t stride, int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    int32_t total = counts[i];
    for (int r = 1; r < replicas; ++r) {
        total += counts[r * stride + i];
        counts[r * stride + i] = 0;
    }
    counts[i] = total;
}

// shade.cl:4-21
__device__ __forceinline__ void heatmap(float intensity, float& r, float& g, float& b)
{
    const float minDosageColor = 0.5f;
    const float upperHalfColor = 0.75f;   // 0.5f + (1.0 - 0.5f) / 2, exact
    const float lowerHalfColor = 0.25f;   // 0.5f / 2.0f, exact
    if (intensity > minDosageColor) {
        if (intensity > upperHalfColor) {
            r = 1.0f; g = (1.0f - intensity) / (1.0f - upperHalfColor); b = 0.0f;
        } else {
            r = (intensity - minDosageColor) / (upperHalfColor - minDosageColor);
            g = 1.0f; b = 0.0f;
        }
    } else {
        if (intensity > lowerHalfColor) {
            r = 0.0f; g = 1.0f;
            b = (minDosageColor - intensity) / (minDosageColor - lowerHalfColor);
        } else {
            r = 0.0f; g = intensity / lowerHalfColor; b = 1.0f;
        }
    }
}

// Batched tracing: per plane the (exact, integer) sum of its deposit replicas -- the int32 payload of the one
// all-reduce of a ray-range-sharded computation -- and the replicas zeroed for the next batch.
__global__ __launch_bounds__(256) void k_fold_planes(int32_t* __restrict__ planes, int32_t* __restrict__ folded,
                                                     int32_t replicas, int32_t T, int prio)
{
    helper_priority(prio);
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int i = g >> 2, part = g & 3;
    int32_t* pl = planes + (int64_t)blockIdx.y * replicas * T;
    int32_t total = 0;
    if (i < T) {
        for (int r = part; r < replicas; r += 4) {
            total += pl[(int64_t)r * T + i];
            pl[(int64_t)r * T + i] = 0;
        }
    }
    total += __builtin_amdgcn_mov_dpp(total, 0xb1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    total += __builtin_amdgcn_mov_dpp(total, 0x4e, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    if (i < T && part == 0) folded[(int64_t)blockIdx.y * T + i] = total;
}

// The sum of a class plane's replicas in use for triangle i, the replicas zeroed: a quad of lanes shares the triangle as above
__device__ __forceinline__ int32_t take_class_plane(int32_t* pl, int32_t replicas, int64_t replica_stride, int i, int part, bool in)
{
    int32_t total = 0;
    if (in) {
        for (int r = part; r < replicas; r += 4) {
            total += pl[(int64_t)r * replica_stride + i];
            pl[(int64_t)r * replica_stride + i] = 0;
        }
    }
    total += __builtin_amdgcn_mov_dpp(total, 0xb1, 0xf, 0xf, true);
    total += __builtin_amdgcn_mov_dpp(total, 0x4e, 0xf, 0xf, true);
    return total;
}

// After k_fold_planes: every class plane of the batch (uvrt_dedupe.h "mask classes") read once per triangle and added to the
// folded plane of each launch its mask holds -- a launch's total is its own plane plus the classes it is a member of.
__global__ __launch_bounds__(256) void k_fold_classes(FoldClassParams p)
{
    helper_priority(p.prio);
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int i = g >> 2, part = g & 3;
    const bool in = i < p.T;
    for (int c = 0; c < p.ncls; ++c) {
        const int32_t total = take_class_plane(p.planes + (int64_t)(p.nplanes + c) * p.plane_stride, p.cls_replicas, p.T, i, part, in);
        if (!in || part != 0 || total == 0) continue;
        for (uint64_t m = p.launches[c]; m != 0ull; m &= m - 1ull) p.folded[(int64_t)__builtin_ctzll(m) * p.T + i] += total;
    }
}

// Replay of a batch in LOGICAL launch order, one quad of lanes per triangle: for every launch the
// reference's accumulate (cl/accumulate.cl:4-14: same f64 additions in the same order, max over the
// per-launch totals) and, where the host loop has a Shade behind it (raytracer.cpp:93-120), computeDosage +
// dosageToColor with that Shade's arguments.  The planes are left zeroed.
__global__ __launch_bounds__(256) void k_replay_batch(ReplayParams p)
{
    helper_priority(p.prio);
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int i = g >> 2, part = g & 3;
    const bool in = i < p.bound;
    double pm = 0, mm = 0;
    if (in && part == 0) { pm = p.photon_map[i]; mm = p.max_map[i]; }
    // the batch's class planes (uvrt_dedupe.h "mask classes"), each read ONCE per triangle: the quad's first lane keeps the
    // totals in LDS and adds to a launch those of the classes it is a member of (a folded batch has them in its planes)
    extern __shared__ int32_t s_cls[];          // [ncls][64 triangles of the workgroup]
    const int ncls = p.is_folded ? 0 : p.ncls;
    for (int c = 0; c < ncls; ++c) {
        const int32_t total = take_class_plane(p.planes + (int64_t)(p.nplanes + c) * p.plane_stride, p.cls_replicas, p.T, i, part, in);
        if (part == 0) s_cls[c * 64 + (threadIdx.x >> 2)] = total;
    }
    for (int k = 0; k < p.count; ++k) {
        const ReplayOp op = p.ops[k];
        int32_t total = 0;
        if (p.is_folded) {
            if (in && part == 0) {
                int32_t* f = p.folded + (int64_t)op.plane * p.T + i;
                total = *f;
                *f = 0;
            }
        } else {
            if (in) {
                int32_t* pl = p.planes + (int64_t)op.plane * p.plane_stride;
                for (int r = part; r < p.replicas; r += 4) {
                    total += pl[(int64_t)r * p.T + i];
                    pl[(int64_t)r * p.T + i] = 0;
                }
            }
            total += __builtin_amdgcn_mov_dpp(total, 0xb1, 0xf, 0xf, true);
            total += __builtin_amdgcn_mov_dpp(total, 0x4e, 0xf, 0xf, true);
        }
        if (!in || part != 0) continue;
        if (ncls > 0)
            for (uint64_t m = p.class_of[k]; m != 0ull; m &= m - 1ull) total += s_cls[__builtin_ctzll(m) * 64 + (threadIdx.x >> 2)];
        const double c = (double)total;                                   // accumulate.cl:9-13
        pm = pm + c * (double)op.duration;
        mm = mm < c ? c : mm;
        if (op.shade) {                                                   // shade.cl:23-41, 43-71
            const double num = (double)op.scaled_power * (op.which_map ? mm : pm);
            const float den = p.area[i] * (float)op.photons_per_light;
            const float dose = (float)(num / (double)den);
            p.dosage[i] = dose;
            const float maxValue = op.min_value * 2;
            const float norm = dose / maxValue;
            float r, gg, b;
            if (op.threshold_view && norm < 0.5f) { r = 0.0f; gg = 0.0f; b = norm * 2.0f; }
            else heatmap(norm, r, gg, b);
            float* col = p.color + (int64_t)i * 9;
            col[0] = r; col[1] = gg; col[2] = b;
            col[3] = r; col[4] = gg; col[5] = b;
            col[6] = r; col[7] = gg; col[8] = b;
        }
    }
    if (in && part == 0) { p.photon_map[i] = pm; p.max_map[i] = mm; }
}

__global__ __launch_bounds__(256) void k_add_counts(int32_t* __restrict__ dst, const int32_t* __restrict__ src, int64_t n)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i < n) dst[i] += src[i];
}

// reset.cl:4-26
__global__ __launch_bounds__(256) void k_reset(double* __restrict__ photon_map,
                                               double* __restrict__ max_map,
                                               int32_t* __restrict__ counts, int32_t replicas,
                                               int64_t stride, float* __restrict__ color,
                                               int32_t reset_color, int32_t T, int prio)
{
    helper_priority(prio);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    photon_map[i] = 0;
    max_map[i] = 0;
    for (int r = 0; r < replicas; ++r) counts[r * stride + i] = 0;
    if (!reset_color) return;
    for (int k = 0; k < 9; ++k) color[(int64_t)i * 9 + k] = 0.0f;
}

// Scene preparation: leaf-ordered triangle records and the per-triangle area of
// shade.cl:33-36 (area = length(cross(v0-v1, v0-v2)) / 2.0f), computed once per scene.
__global__ __launch_bounds__(256) void k_prepare_scene(const float4* __restrict__ tris64,
                                                       const uint32_t* __restrict__ tri_idx,
                                                       LeafTri* __restrict__ ltris,
                                                       float* __restrict__ area, int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    {
        const uint32_t id = tri_idx[i];
        const float4 v0 = tris64[(int64_t)id * 4 + 0], v1 = tris64[(int64_t)id * 4 + 1],
                     v2 = tris64[(int64_t)id * 4 + 2];
        LeafTri t;
        t.v0_id = make_float4(v0.x, v0.y, v0.z, __uint_as_float(id));
        t.e1 = make_float4(v1.x - v0.x, v1.y - v0.y, v1.z - v0.z, 0.0f);
        t.e2 = make_float4(v2.x - v0.x, v2.y - v0.y, v2.z - v0.z, 0.0f);
        ltris[i] = t;
    }
    {
        const float4 v0 = tris64[(int64_t)i * 4 + 0], v1 = tris64[(int64_t)i * 4 + 1],
                     v2 = tris64[(int64_t)i * 4 + 2];
        const float ax = v0.x - v1.x, ay = v0.y - v1.y, az = v0.z - v1.z;
        const float bx = v0.x - v2.x, by = v0.y - v2.y, bz = v0.z - v2.z;
        const float cx = ay * bz - az * by;
        const float cy = az * bx - ax * bz;
        const float cz = ax * by - ay * bx;
        area[i] = sqrtf(cx * cx + cy * cy + cz * cz) / 2.0f;
    }
}

// shade.cl:23-41: dose = (scaledPower * photonMap) / (area * photonsPerLight)
//   f32*f64 -> f64 ; f32*(int->f32) -> f32 ; f64/f32 -> f64 ; narrowed to f32
__global__ __launch_bounds__(256) void k_compute_dosage(const double* __restrict__ map,
                                                        float* __restrict__ dosage,
                                                        const float* __restrict__ area,
                                                        int32_t photons_per_light,
                                                        float scaled_power, int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const double num = (double)scaled_power * map[i];
    const float den = area[i] * (float)photons_per_light;
    dosage[i] = (float)(num / (double)den);
}

// shade.cl:43-71
__global__ __launch_bounds__(256) void k_dosage_to_color(const float* __restrict__ dosage,
                                                         float* __restrict__ color,
                                                         float min_value, int32_t threshold_view,
                                                         int32_t T)
{
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    const float maxValue = min_value * 2;
    const float norm = dosage[i] / maxValue;
    float r, g, b;
    if (threshold_view && norm < 0.5f) { r = 0.0f; g = 0.0f; b = norm * 2.0f; }
    else heatmap(norm, r, g, b);
    float* c = color + (int64_t)i * 9;
    c[0] = r; c[1] = g; c[2] = b;
    c[3] = r; c[4] = g; c[5] = b;
    c[6] = r; c[7] = g; c[8] = b;
}

// computeDosage + dosageToColor of triangle i from its map value (shade.cl:23-71); the dose still goes through its f32 store
__device__ __forceinline__ void shade_one(int i, double map_value, float* __restrict__ dosage, const float* __restrict__ area,
                                          float* __restrict__ color, int32_t photons_per_light, float scaled_power,
                                          float min_value, int32_t threshold_view)
{
    const double num = (double)scaled_power * map_value;                // shade.cl:39
    const float den = area[i] * (float)photons_per_light;
    const float dose = (float)(num / (double)den);
    dosage[i] = dose;
    const float maxValue = min_value * 2;                               // shade.cl:47-50
    const float norm = dose / maxValue;
    float r, g, b;
    if (threshold_view && norm < 0.5f) { r = 0.0f; g = 0.0f; b = norm * 2.0f; }
    else heatmap(norm, r, g, b);
    float* c = color + (int64_t)i * 9;
    c[0] = r; c[1] = g; c[2] = b;
    c[3] = r; c[4] = g; c[5] = b;
    c[6] = r; c[7] = g; c[8] = b;
}

// computeDosage + dosageToColor in one pass (RayTracer::Shade always runs them back to back,
// raytracer.cpp:93-120); same operations
__global__ __launch_bounds__(256) void k_shade(const double* __restrict__ map, float* __restrict__ dosage,
                                               const float* __restrict__ area, float* __restrict__ color,
                                               int32_t photons_per_light, float scaled_power,
                                               float min_value, int32_t threshold_view, int32_t T, int prio)
{
    helper_priority(prio);
    const int i = blockIdx.x * 256 + threadIdx.x;
    if (i >= T) return;
    shade_one(i, map[i], dosage, area, color, photons_per_light, scaled_power, min_value, threshold_view);
}

// accumulate.cl:4-14 of the launch just traced and the Shade that the host loop runs right after it (myapp.cpp:159-160)
// in ONE launch: k_accumulate's fold of the deposit replicas and its map update, then shade_one on the value just written.
// which_map: 0 photonMap, 1 maxPhotonMap.
__global__ __launch_bounds__(256) void k_accumulate_shade(double* __restrict__ photon_map, double* __restrict__ max_map,
                                                          int32_t* __restrict__ counts, int32_t replicas, int64_t stride,
                                                          float time_step, float* __restrict__ dosage,
                                                          const float* __restrict__ area, float* __restrict__ color,
                                                          int32_t which_map, int32_t photons_per_light, float scaled_power,
                                                          float min_value, int32_t threshold_view, int32_t T, int prio)
{
    helper_priority(prio);
    const int g = blockIdx.x * 256 + threadIdx.x;
    const int i = g >> 2, part = g & 3;
    int32_t total = 0;
    if (i < T) {
        for (int r = part; r < replicas; r += 4) {
            total += counts[r * stride + i];
            counts[r * stride + i] = 0;
        }
    }
    total += __builtin_amdgcn_mov_dpp(total, 0xb1, 0xf, 0xf, true);   // quad_perm [1,0,3,2]
    total += __builtin_amdgcn_mov_dpp(total, 0x4e, 0xf, 0xf, true);   // quad_perm [2,3,0,1]
    if (i >= T || part != 0) return;
    const double c = (double)total;
    const double sum = photon_map[i] + c * (double)time_step;          // accumulate.cl:9
    photon_map[i] = sum;
    const double m = max_map[i];
    const double mx = m < c ? c : m;                                    // accumulate.cl:11
    max_map[i] = mx;
    shade_one(i, which_map ? mx : sum, dosage, area, color, photons_per_light, scaled_power, min_value, threshold_view);
}

// Measurement hook (uvrt_clock_probe_start): one wave reads the shader-clock counter (s_memtime) and the constant 100 MHz counter
// (s_memrealtime) `ticks` of the latter apart, sleeping in between; out = {shader ticks, 100 MHz ticks}.  Launched on a stream of
// its own beside whatever the device is doing, it tells what the shader clock IS under that load (the issue-rate peaks of the
// bench line's roofline scale with it; it moves between 2.0 and 2.4 GHz with the power the load draws).
__global__ __launch_bounds__(64) void k_clock_probe(unsigned long long* out, unsigned long long ticks)
{
    const unsigned long long r0 = __builtin_amdgcn_s_memrealtime();
    const unsigned long long t0 = __builtin_amdgcn_s_memtime();
    unsigned long long r1 = r0;
    while (r1 - r0 < ticks) {
        __builtin_amdgcn_s_sleep(32);
        r1 = __builtin_amdgcn_s_memrealtime();
    }
    const unsigned long long t1 = __builtin_amdgcn_s_memtime();
    r1 = __builtin_amdgcn_s_memrealtime();
    if (threadIdx.x == 0) { out[0] = t1 - t0; out[1] = r1 - r0; }
}

void launch_clock_probe(unsigned long long* out, unsigned long long ticks, hipStream_t s)
{
    hipLaunchKernelGGL(k_clock_probe, dim3(1), dim3(64), 0, s, out, ticks);
}

// Test hook: the reference's 32-byte Ray records (cl/tools.cl:8-14) in gid order.
__global__ __launch_bounds__(256) void k_export_rays(const float4* __restrict__ rays,
                                                     const uint2* __restrict__ hits,
                                                     float4* __restrict__ out, float ox,
                                                     float oz, int64_t first, int64_t count)
{
    const int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x;
    if (i >= count) return;
    const float4 rec = rays[first + i];
    uint2 h = make_uint2(__float_as_uint(1e30f), 0u);
    if (hits) h = hits[first + i];
    out[i * 2 + 0] = make_float4(rec.x, rec.y, rec.z, ox);
    out[i * 2 + 1] = make_float4(rec.w, oz, __uint_as_float(h.x), __uint_as_float(h.y));
}

// ------------------------------------------------------------------------ launch wrappers

static inline unsigned blocks_for(int64_t n, int per) { return (unsigned)((n + per - 1) / per); }

void launch_generate(const GenParams& p0, hipStream_t s)
{
    GenParams p = p0;
    p.ray_blocks = p.n > 0 ? blocks_for(p.n, 256) : 0u;
    const unsigned prep_blocks = p.prep_recs ? blocks_for(p.prep_npairs, 256) : 0u;
    if (p.ray_blocks + prep_blocks == 0) return;
    hipLaunchKernelGGL(k_generate, dim3(p.ray_blocks + prep_blocks), dim3(256), 0, s, p);
}

void launch_generate_batch(const GenBatchParams& p, hipStream_t s)
{
    if (p.n <= 0 || p.count <= 0) return;
    hipLaunchKernelGGL(k_generate_batch, dim3(blocks_for(p.n, 256), (unsigned)p.count), dim3(256), 0, s, p);
}

void launch_dedupe_mark(const GenDedupeParams& p, hipStream_t s)
{
    if (p.gn <= 0 || p.g.count <= 0 || (p.gaps <= 0 && p.per.count <= 0) || p.strip_tiles <= 0) return;
    // the strips of the gaps, and with a period table a thread per launch and block of DD_SLOTS gids for the interiors' owners
    const unsigned count_groups = p.per.count > 0 ? blocks_for((int64_t)p.g.count * blocks_for(p.gn, DD_SLOTS), 64) : 0u;
    hipLaunchKernelGGL(k_dedupe_mark, dim3((unsigned)p.gap_strip0[p.gaps] + count_groups), dim3(64), 0, s, p);
}

void launch_generate_dedupe(const GenDedupeParams& p, hipStream_t s)
{
    if (p.gn <= 0 || p.g.count <= 0) return;
    const dim3 grid(blocks_for(p.gn, DD_SLOTS), (unsigned)p.g.count);
    launch_dedupe_mark(p, s);
    hipLaunchKernelGGL(k_dedupe_scan, dim3(1), dim3(256), 0, s, p.block_counts, p.total, p.deposits, grid.x * grid.y, (int)p.prio);
    hipLaunchKernelGGL(k_dedupe_write, grid, dim3(256), 0, s, p);
}

void launch_fold_planes(int32_t* planes, int32_t* folded, int32_t nplanes, int32_t replicas, int32_t T, int prio, hipStream_t s)
{
    if (nplanes <= 0 || T <= 0) return;
    hipLaunchKernelGGL(k_fold_planes, dim3(blocks_for((int64_t)T * 4, 256), (unsigned)nplanes), dim3(256), 0, s, planes,
                       folded, replicas, T, prio);
}

void launch_replay_batch(const ReplayParams& p, hipStream_t s)
{
    if (p.count <= 0 || p.bound <= 0) return;
    const size_t lds = p.is_folded ? 0 : (size_t)p.ncls * 64 * sizeof(int32_t);      // (the class totals of the workgroup's triangles)
    hipLaunchKernelGGL(k_replay_batch, dim3(blocks_for((int64_t)p.bound * 4, 256)), dim3(256), lds, s, p);
}

void launch_fold_classes(const FoldClassParams& p, hipStream_t s)
{
    if (p.ncls <= 0 || p.T <= 0) return;
    hipLaunchKernelGGL(k_fold_classes, dim3(blocks_for((int64_t)p.T * 4, 256)), dim3(256), 0, s, p);
}

void launch_add_counts(int32_t* dst, const int32_t* src, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_add_counts, dim3(blocks_for(n, 256)), dim3(256), 0, s, dst, src, n);
}

void launch_scan_bins(uint32_t* hist, uint32_t* bin_start, int32_t nbins, hipStream_t s)
{
    hipLaunchKernelGGL(k_scan_bins, dim3(1), dim3(1024), 0, s, hist, bin_start, nbins);
}

void launch_scatter(const float4* rays, const uint2* keyrank, const uint32_t* bin_start,
                    float4* sorted, uint32_t* order, int64_t n, hipStream_t s)
{
    if (n <= 0) return;
    hipLaunchKernelGGL(k_scatter, dim3(blocks_for(n, 256)), dim3(256), 0, s, rays, keyrank,
                       bin_start, sorted, order, n);
}

void launch_accumulate(double* photon_map, double* max_map, int32_t* counts, int32_t replicas,
                       int64_t stride, float time_step, int32_t T, int prio, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_accumulate, dim3(blocks_for((int64_t)T * 4, 256)), dim3(256), 0, s, photon_map,
                       max_map, counts, replicas, stride, time_step, T, prio);
}

void launch_fold_counts(int32_t* counts, int32_t replicas, int64_t stride, int32_t T, hipStream_t s)
{
    if (T <= 0 || replicas <= 1) return;
    hipLaunchKernelGGL(k_fold_counts, dim3(blocks_for(T, 256)), dim3(256), 0, s, counts, replicas,
                       stride, T);
}

void launch_reset(double* photon_map, double* max_map, int32_t* counts, int32_t replicas,
                  int64_t stride, float* color, int32_t reset_color, int32_t T, int prio, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_reset, dim3(blocks_for(T, 256)), dim3(256), 0, s, photon_map, max_map,
                       counts, replicas, stride, color, reset_color, T, prio);
}

void launch_compute_dosage(const double* map, float* dosage, const float* area,
                           int32_t photons_per_light, float scaled_power, int32_t T,
                           hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_compute_dosage, dim3(blocks_for(T, 256)), dim3(256), 0, s, map, dosage,
                       area, photons_per_light, scaled_power, T);
}

void launch_shade(const double* map, float* dosage, const float* area, float* color, int32_t photons_per_light,
                  float scaled_power, float min_value, int32_t threshold_view, int32_t T, int prio, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_shade, dim3(blocks_for(T, 256)), dim3(256), 0, s, map, dosage, area, color,
                       photons_per_light, scaled_power, min_value, threshold_view, T, prio);
}

void launch_accumulate_shade(double* photon_map, double* max_map, int32_t* counts, int32_t replicas, int64_t stride,
                             float time_step, float* dosage, const float* area, float* color, int32_t which_map,
                             int32_t photons_per_light, float scaled_power, float min_value, int32_t threshold_view,
                             int32_t T, int prio, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_accumulate_shade, dim3(blocks_for((int64_t)T * 4, 256)), dim3(256), 0, s, photon_map, max_map, counts,
                       replicas, stride, time_step, dosage, area, color, which_map, photons_per_light, scaled_power, min_value,
                       threshold_view, T, prio);
}

void launch_dosage_to_color(const float* dosage, float* color, float min_value,
                            int32_t threshold_view, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_dosage_to_color, dim3(blocks_for(T, 256)), dim3(256), 0, s, dosage,
                       color, min_value, threshold_view, T);
}

void launch_prepare_scene(const float4* tris64, const uint32_t* tri_idx, LeafTri* ltris,
                          float* area, int32_t T, hipStream_t s)
{
    if (T <= 0) return;
    hipLaunchKernelGGL(k_prepare_scene, dim3(blocks_for(T, 256)), dim3(256), 0, s, tris64,
                       tri_idx, ltris, area, T);
}

void launch_export_rays(const float4* rays, const uint2* hits, void* out32, float ox, float oz,
                        int64_t first, int64_t count, hipStream_t s)
{
    if (count <= 0) return;
    hipLaunchKernelGGL(k_export_rays, dim3(blocks_for(count, 256)), dim3(256), 0, s, rays, hits,
                       (float4*)out32, ox, oz, first, count);
}

}  // namespace uvrt

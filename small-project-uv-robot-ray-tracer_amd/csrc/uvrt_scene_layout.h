// uvrt_scene_layout.h -- the re-layout of a scene, worked out on the host before anything touches the GPU: the reference's
// BVH2 breadth-first into pair records, its one-level 4-wide collapse into quad records, the leaves' triangle counts, the
// root reference, the two prefixes the traversals cache, and whether the scene is outside the reciprocal shortcuts' proofs.
// A function of uvrt_set_scene's arguments alone: no HIP, so tests/tools/scene_layout_check.cpp runs it in a g++ build.
// uvrt_capi.hip uploads the records' bytes; it holds the static_asserts that tie the records and constants below to
// uvrt_device.h's PairRec, QuadRec, REF_*, TOP6_MAX and MAX_TRIS.
#pragma once
#include "../../include/uvrt.h"

#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <string>
#include <vector>

namespace uvrt {
namespace scene_layout {

// (uvrt_device.h's, by the same names)
constexpr uint32_t REF_LEAF_BIT = 0x80000000u;
constexpr uint32_t REF_DONE = 0xFFFFFFFFu;
constexpr int REF_COUNT_SHIFT = 27;
constexpr int MAX_TRIS = 1 << 27;
constexpr uint32_t TOP6_MAX = 175;

struct F4 { float x, y, z, w; };
inline F4 f4(float x, float y, float z, float w) { return F4{x, y, z, w}; }

struct PairWords {             // PairRec, 16 words
    F4 c0min_ref0;             // child0 min.xyz, bits of ref0
    F4 c0max_ref1;             // child0 max.xyz, bits of ref1
    F4 c1min;                  // child1 min.xyz, 0
    F4 c1max;                  // child1 max.xyz, 0
};
struct QuadWords {             // QuadRec, 32 words
    F4 xz[4];                  // child k: min.x, max.x, min.z, max.z
    F4 y01, y23;               // c0 min.y, c0 max.y, c1 min.y, c1 max.y ; likewise c2, c3
    uint32_t ref[4];           // inner: unit index (2 x node index); leaf: as in the BVH2 form
    uint32_t pad[4];
};
static_assert(sizeof(PairWords) == 64 && sizeof(QuadWords) == 128, "16 and 32 four-byte words");

struct HostNode { float mn[3]; int32_t leftFirst; float mx[3]; int32_t triCount; };
static_assert(sizeof(HostNode) == 32, "BVHNode is 32 bytes (bvh.h:11-21)");

struct SceneLayout {
    std::vector<PairWords> pairs;          // one per inner node, breadth-first from node 0
    std::vector<QuadWords> quads;          // one per node of the 4-wide collapse, breadth-first
    std::vector<uint32_t> leaf_count;      // [T]: triangles of the leaf that starts at the slot
    uint32_t root_ref = REF_DONE;          // 0, or the root's leaf reference
    uint32_t top_pairs = 0;                // pairs [0, top_pairs): tree depths 0..7, TOP6_MAX at most
    uint32_t top_quads = 0;                // quads [0, top_quads): depths 0..3 of the collapse, 64 at most
    bool force_exact = false;              // a bound or a vertex outside the reciprocal shortcuts' range proofs
};

inline int layout_fail(std::string& why, int code, const char* fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof buf, fmt, ap);
    va_end(ap);
    why = buf;
    return code;
}

// vertex coordinates beyond 1e9 (or non-finite): the shortcuts' range proofs do not cover them
inline bool has_huge_vertex(const void* tris64, int32_t T)
{
    const float* tv = (const float*)tris64;
    for (int64_t i = 0; i < (int64_t)T; ++i)
        for (int k = 0; k < 12; ++k)
            if ((k & 3) != 3 && !(std::fabs(tv[i * 16 + k]) <= 1e9f)) return true;
    return false;
}

inline uint32_t leaf_ref(const HostNode& n, int32_t T, std::vector<uint32_t>& leaf_count, int& err)
{
    int64_t first = n.leftFirst, cnt = n.triCount;
    if (first < 0 || first + cnt > T) { err = 1; return REF_DONE; }
    leaf_count[first] = (uint32_t)cnt;
    uint32_t code = cnt >= 15 ? 15u : (uint32_t)cnt;
    return REF_LEAF_BIT | (code << REF_COUNT_SHIFT) | (uint32_t)first;
}

// Walks the tree breadth-first from node 0; every inner node becomes one pair record (numbered in visit order, so the
// top of the tree is contiguous at the front).  Returns the malformed-BVH code, 0 for none; sets `tiny_bound`.
inline int build_pairs(const HostNode* nodes, int32_t node_count, int32_t T, SceneLayout& L, bool& tiny_bound)
{
    std::vector<PairWords>& pairs = L.pairs;
    std::vector<int32_t> queue;   // inner nodes in BFS order; index in queue == pair index
    std::vector<int32_t> depth;   // tree depth of queue[i]
    int err = 0;
    if (nodes[0].triCount > 0) {
        L.root_ref = leaf_ref(nodes[0], T, L.leaf_count, err);
    } else {
        L.root_ref = 0;
        queue.push_back(0);
        depth.push_back(0);
    }
    for (size_t qi = 0; qi < queue.size() && !err; ++qi) {
        const HostNode& n = nodes[queue[qi]];
        const int64_t l = n.leftFirst;
        if (l < 0 || l + 1 >= node_count) { err = 2; break; }
        if (queue.size() > (size_t)node_count) { err = 3; break; }   // cycle
        uint32_t ref[2];
        for (int k = 0; k < 2; ++k) {
            const HostNode& ch = nodes[l + k];
            if (ch.triCount > 0) ref[k] = leaf_ref(ch, T, L.leaf_count, err);
            else { ref[k] = (uint32_t)queue.size(); queue.push_back((int32_t)(l + k)); depth.push_back(depth[qi] + 1); }
        }
        const HostNode& a = nodes[l];
        const HostNode& b = nodes[l + 1];
        for (const HostNode* hn : {&a, &b})
            for (int k = 0; k < 3; ++k)
                for (float v : {hn->mn[k], hn->mx[k]})
                    if ((v != 0.0f && std::fabs(v) < 8.6736174e-19f) || !(std::fabs(v) <= 1e9f))
                        tiny_bound = true;   // below 2^-60, above 1e9, inf or NaN
        PairWords pr;
        pr.c0min_ref0 = f4(a.mn[0], a.mn[1], a.mn[2], 0.f);
        pr.c0max_ref1 = f4(a.mx[0], a.mx[1], a.mx[2], 0.f);
        memcpy(&pr.c0min_ref0.w, &ref[0], 4);
        memcpy(&pr.c0max_ref1.w, &ref[1], 4);
        pr.c1min = f4(b.mn[0], b.mn[1], b.mn[2], 0.f);
        pr.c1max = f4(b.mx[0], b.mx[1], b.mx[2], 0.f);
        pairs.push_back(pr);
        if (depth[qi] < 8 && L.top_pairs < TOP6_MAX) L.top_pairs = (uint32_t)qi + 1;   // level order: a prefix
    }
    return err;
}

// a child of a 4-wide node while it is put together
struct QuadChild { float mn[3], mx[3]; uint32_t ref; };
inline void add(QuadChild ch[4], int& nch, const F4& mn, const F4& mx, uint32_t ref)
{
    QuadChild& c4 = ch[nch++];
    c4.mn[0] = mn.x; c4.mn[1] = mn.y; c4.mn[2] = mn.z;
    c4.mx[0] = mx.x; c4.mx[1] = mx.y; c4.mx[2] = mx.z;
    c4.ref = ref;
}
inline void children_of(const PairWords& pr, F4 mn[2], F4 mx[2], uint32_t ref[2])
{
    mn[0] = pr.c0min_ref0; mx[0] = pr.c0max_ref1; mn[1] = pr.c1min; mx[1] = pr.c1max;
    memcpy(&ref[0], &pr.c0min_ref0.w, 4);
    memcpy(&ref[1], &pr.c0max_ref1.w, 4);
}

// The 4-wide collapse (one level): a node takes the children of its inner children.  Numbered breadth-first
// like the pairs; a child reference is a 64-byte unit index (2 x node index) or the BVH2 leaf reference.
inline void build_quads(SceneLayout& L)
{
    const std::vector<PairWords>& pairs = L.pairs;
    std::vector<QuadWords>& quads = L.quads;
    if (pairs.empty()) return;
    std::vector<int32_t> qpair{0};        // pair index (of the BVH2 inner node) of every 4-wide node
    std::vector<int32_t> qdepth{0};
    const float far_box = 1e30f;          // an empty slot: a box no ray reaches (entry distance >= 1e30)
    for (size_t qi = 0; qi < qpair.size(); ++qi) {
        QuadChild ch[4];
        int nch = 0;
        F4 mn[2], mx[2];
        uint32_t ref[2];
        children_of(pairs[qpair[qi]], mn, mx, ref);
        for (int k = 0; k < 2; ++k) {
            if (ref[k] >= REF_LEAF_BIT) { add(ch, nch, mn[k], mx[k], ref[k]); continue; }
            F4 gmn[2], gmx[2];
            uint32_t gref[2];
            children_of(pairs[ref[k]], gmn, gmx, gref);
            for (int j = 0; j < 2; ++j) add(ch, nch, gmn[j], gmx[j], gref[j]);
        }
        QuadWords q;
        memset(&q, 0, sizeof q);
        float y[4][2];
        for (int k = 0; k < 4; ++k) {
            if (k < nch) {
                uint32_t r = ch[k].ref;
                if (r < REF_LEAF_BIT) {           // inner: it becomes a 4-wide node of its own
                    qpair.push_back((int32_t)r);
                    qdepth.push_back(qdepth[qi] + 1);
                    r = 2u * (uint32_t)(qpair.size() - 1);
                }
                q.xz[k] = f4(ch[k].mn[0], ch[k].mx[0], ch[k].mn[2], ch[k].mx[2]);
                y[k][0] = ch[k].mn[1]; y[k][1] = ch[k].mx[1];
                q.ref[k] = r;
            } else {
                q.xz[k] = f4(far_box, far_box, far_box, far_box);
                y[k][0] = y[k][1] = far_box;
                q.ref[k] = REF_DONE;
            }
        }
        q.y01 = f4(y[0][0], y[0][1], y[1][0], y[1][1]);
        q.y23 = f4(y[2][0], y[2][1], y[3][0], y[3][1]);
        quads.push_back(q);
        if (qdepth[qi] < 4 && L.top_quads < 64) L.top_quads = (uint32_t)qi + 1;     // levels 0-3: up to 85 nodes, 64 cached
    }
}

// uvrt_set_scene's arguments into a SceneLayout, or its refusal: the code, and the text in `why`
inline int build_scene_layout(const void* tris64, int32_t T, const void* nodes32, int32_t node_count, const uint32_t* tri_idx,
                              SceneLayout& L, std::string& why)
{
    if (!tris64 || !nodes32 || !tri_idx) return layout_fail(why, UVRT_ERR_INVALID, "uvrt_set_scene: null argument");
    if (T <= 0 || T > MAX_TRIS || node_count <= 0)
        return layout_fail(why, UVRT_ERR_INVALID, "uvrt_set_scene: tri_count %d / node_count %d out of range", T, node_count);
    for (int32_t i = 0; i < T; ++i)
        if (tri_idx[i] >= (uint32_t)T)
            return layout_fail(why, UVRT_ERR_BVH, "uvrt_set_scene: triIdx[%d] = %u >= tri_count %d", i, tri_idx[i], T);
    const bool huge_vertex = has_huge_vertex(tris64, T);
    L = SceneLayout();
    L.leaf_count.assign((size_t)T, 0u);
    bool tiny_bound = false;
    if (int err = build_pairs((const HostNode*)nodes32, node_count, T, L, tiny_bound))
        return layout_fail(why, UVRT_ERR_BVH, "uvrt_set_scene: malformed BVH (code %d)", err);
    build_quads(L);
    // a child reference is a record index with 32-bit byte offsets: inner-node records + leaf records < 2^26
    if (L.pairs.size() + (size_t)T >= ((size_t)1 << 26))
        return layout_fail(why, UVRT_ERR_INVALID, "uvrt_set_scene: %zu inner nodes + %d triangles exceed 2^26 records", L.pairs.size(), T);
    L.force_exact = tiny_bound || huge_vertex;
    return UVRT_OK;
}

}  // namespace scene_layout
}  // namespace uvrt

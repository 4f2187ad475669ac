// scene_layout_check.cpp -- csrc/uvrt_scene_layout.h alone in a g++ build (tests/test_scene_layout_cpu.py):
//   scene_layout_check <scene file> <layout file>
// reads a scene, runs build_scene_layout, writes what it returned, and holds the layout to the invariants that need no
// restatement: every inner node reachable from the root is one pair record, in breadth-first order; every reference is a
// pair index or has the leaf bit; the quads reach exactly the pairs' leaf references; top_pairs and top_quads are prefixes.
// Prints one line per breach and "<n> breaches"; exit status 0 only with none.
//
// scene file:  int32 T, node_count, nodes stored, triIdx entries stored; float[T][16]; BVHNode[stored]; uint32[stored]
// layout file: int32 code; then for code 0: uint32 npairs, nquads, root_ref, top_pairs, top_quads, force_exact;
//              the pair records; the quad records; uint32 leaf_count[T] -- else the refusal's text
#include "uvrt_scene_layout.h"

#include <algorithm>
#include <cstdlib>

using namespace uvrt::scene_layout;

static int breaches = 0;
#define CHECK(cond, ...)                                        \
    do {                                                        \
        if (!(cond)) {                                          \
            if (++breaches <= 20) { printf("breach: " __VA_ARGS__); printf("\n"); } \
        }                                                       \
    } while (0)

static uint32_t bits(float f) { uint32_t u; memcpy(&u, &f, 4); return u; }

static void check_pairs(const SceneLayout& L, const HostNode* nodes)
{
    const size_t P = L.pairs.size();
    if (L.root_ref != 0) {
        CHECK(L.root_ref >= REF_LEAF_BIT && P == 0, "a leaf root with %zu pairs", P);
        return;
    }
    // the inner nodes by a walk of our own: pair i is node order[i]
    std::vector<int32_t> order{0};
    std::vector<int> depth{0};
    for (size_t i = 0; i < order.size() && i < P; ++i) {
        const int32_t l = nodes[order[i]].leftFirst;
        const PairWords& pr = L.pairs[i];
        const uint32_t ref[2] = {bits(pr.c0min_ref0.w), bits(pr.c0max_ref1.w)};
        const F4* mn[2] = {&pr.c0min_ref0, &pr.c1min};
        const F4* mx[2] = {&pr.c0max_ref1, &pr.c1max};
        for (int k = 0; k < 2; ++k) {
            const HostNode& ch = nodes[l + k];
            CHECK(memcmp(mn[k], ch.mn, 12) == 0 && memcmp(mx[k], ch.mx, 12) == 0, "pair %zu child %d: not node %d's box", i, k, l + k);
            CHECK(ref[k] < P || ref[k] >= REF_LEAF_BIT, "pair %zu ref %d = %08x: neither a pair nor a leaf", i, k, ref[k]);
            if (ch.triCount > 0) {
                CHECK(ref[k] >= REF_LEAF_BIT && (ref[k] & 0x07FFFFFFu) == (uint32_t)ch.leftFirst, "pair %zu ref %d: not leaf %d", i, k, l + k);
            } else {
                CHECK(ref[k] == order.size(), "pair %zu ref %d = %u: the next inner node is %zu", i, k, ref[k], order.size());
                order.push_back(l + k);
                depth.push_back(depth[i] + 1);
            }
        }
        CHECK(bits(pr.c1min.w) == 0 && bits(pr.c1max.w) == 0, "pair %zu: padding words", i);
    }
    CHECK(order.size() == P, "%zu inner nodes reachable, %zu pairs", order.size(), P);
    std::vector<int32_t> once(order);
    std::sort(once.begin(), once.end());
    CHECK(std::adjacent_find(once.begin(), once.end()) == once.end(), "an inner node appears twice");
    const size_t tp = L.top_pairs;
    CHECK(tp <= P && tp <= TOP6_MAX && (P == 0 || tp >= 1), "top_pairs %zu of %zu", tp, P);
    for (size_t i = 0; i < tp && i < depth.size(); ++i) CHECK(depth[i] < 8, "pair %zu in the prefix at depth %d", i, depth[i]);
    if (tp < TOP6_MAX && tp < depth.size()) CHECK(depth[tp] >= 8, "pair %zu at depth %d left out of the prefix", tp, depth[tp]);
}

static void check_quads(const SceneLayout& L)
{
    const size_t P = L.pairs.size(), Q = L.quads.size();
    CHECK((P == 0) == (Q == 0), "%zu pairs, %zu quads", P, Q);
    std::vector<uint32_t> pair_leaves, quad_leaves;
    for (const PairWords& pr : L.pairs)
        for (uint32_t r : {bits(pr.c0min_ref0.w), bits(pr.c0max_ref1.w)})
            if (r >= REF_LEAF_BIT) pair_leaves.push_back(r);
    std::vector<int> qdepth(Q, -1);
    if (Q) qdepth[0] = 0;
    size_t next = 1;                           // breadth-first: the inner children are numbered in visit order
    for (size_t i = 0; i < Q; ++i) {
        const QuadWords& q = L.quads[i];
        CHECK(qdepth[i] >= 0, "quad %zu: no parent", i);
        bool empty = false;
        for (int k = 0; k < 4; ++k) {
            const uint32_t r = q.ref[k];
            CHECK(q.pad[k] == 0, "quad %zu: padding words", i);
            if (r == REF_DONE) {
                empty = true;
                CHECK(q.xz[k].x == 1e30f && q.xz[k].y == 1e30f && q.xz[k].z == 1e30f && q.xz[k].w == 1e30f, "quad %zu slot %d: not the far box", i, k);
                continue;
            }
            CHECK(!empty, "quad %zu: a child behind an empty slot", i);
            if (r >= REF_LEAF_BIT) { quad_leaves.push_back(r); continue; }
            CHECK((r & 1u) == 0 && r / 2 == next && next < Q, "quad %zu ref %d = %u: the next node is %zu of %zu", i, k, r, next, Q);
            if (r / 2 < Q) qdepth[r / 2] = qdepth[i] + 1;
            ++next;
        }
    }
    CHECK(next == Q || Q == 0, "%zu quads reached of %zu", next, Q);
    std::sort(pair_leaves.begin(), pair_leaves.end());
    std::sort(quad_leaves.begin(), quad_leaves.end());
    CHECK(pair_leaves == quad_leaves, "the quads reach %zu leaves, the pairs hold %zu", quad_leaves.size(), pair_leaves.size());
    const size_t tq = L.top_quads;
    CHECK(tq <= Q && tq <= 64 && (Q == 0 || tq >= 1), "top_quads %zu of %zu", tq, Q);
    for (size_t i = 0; i < tq; ++i) CHECK(qdepth[i] < 4, "quad %zu in the prefix at depth %d", i, qdepth[i]);
    if (tq < 64 && tq < Q) CHECK(qdepth[tq] >= 4, "quad %zu at depth %d left out of the prefix", tq, qdepth[tq]);
}

int main(int argc, char** argv)
{
    if (argc != 3) { fprintf(stderr, "usage: %s <scene file> <layout file>\n", argv[0]); return 2; }
    FILE* in = fopen(argv[1], "rb");
    if (!in) { perror(argv[1]); return 2; }
    int32_t hdr[4];
    if (fread(hdr, 4, 4, in) != 4 || hdr[0] < 0 || hdr[2] < 0 || hdr[3] < 0) { fprintf(stderr, "bad header\n"); return 2; }
    const int32_t T = hdr[0], node_count = hdr[1];
    std::vector<float> tris((size_t)T * 16 + 1);
    std::vector<HostNode> nodes((size_t)hdr[2] + 1);
    std::vector<uint32_t> idx((size_t)hdr[3] + 1);
    if (fread(tris.data(), 64, (size_t)T, in) != (size_t)T || fread(nodes.data(), 32, (size_t)hdr[2], in) != (size_t)hdr[2] ||
        fread(idx.data(), 4, (size_t)hdr[3], in) != (size_t)hdr[3]) { fprintf(stderr, "short scene file\n"); return 2; }
    fclose(in);
    if (node_count > hdr[2] || T > hdr[3]) { fprintf(stderr, "the file holds fewer nodes / entries than it names\n"); return 2; }

    SceneLayout L;
    std::string why;
    const int32_t rc = build_scene_layout(tris.data(), T, nodes.data(), node_count, idx.data(), L, why);
    FILE* out = fopen(argv[2], "wb");
    if (!out) { perror(argv[2]); return 2; }
    fwrite(&rc, 4, 1, out);
    if (rc != UVRT_OK) {
        fwrite(why.data(), 1, why.size(), out);
    } else {
        const uint32_t head[6] = {(uint32_t)L.pairs.size(), (uint32_t)L.quads.size(), L.root_ref, L.top_pairs, L.top_quads,
                                  L.force_exact ? 1u : 0u};
        fwrite(head, 4, 6, out);
        if (!L.pairs.empty()) fwrite(L.pairs.data(), sizeof(PairWords), L.pairs.size(), out);      // (a leaf root: neither)
        if (!L.quads.empty()) fwrite(L.quads.data(), sizeof(QuadWords), L.quads.size(), out);
        fwrite(L.leaf_count.data(), 4, L.leaf_count.size(), out);
        CHECK(L.leaf_count.size() == (size_t)T, "leaf_count holds %zu entries", L.leaf_count.size());
        check_pairs(L, nodes.data());
        check_quads(L);
    }
    fclose(out);
    printf("code %d%s%s\n%d breaches\n", rc, rc ? ": " : "", why.c_str(), breaches);
    return breaches ? 1 : 0;
}

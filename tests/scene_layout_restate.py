"""What uvrt_set_scene makes of a scene before it touches the GPU (csrc/uvrt_scene_layout.h), restated in numpy: the
numbering of the pair records, their words, the 4-wide collapse's words, leaf_count, root_ref, the two cached prefixes and
the flag that keeps a scene off the reciprocal shortcuts.  pair_order is the one statement of the numbering for the tests
and the tools under tests/tools; layout() is what tests/test_scene_layout_cpu.py compares build_scene_layout with, word
for word."""
import numpy as np

REF_LEAF_BIT = 0x80000000
REF_DONE = 0xFFFFFFFF
REF_COUNT_SHIFT = 27
TOP6_MAX = 175          # pair records the traversal serves from LDS (uvrt_device.h)
TOP_QUADS_MAX = 64
FAR_BOX = np.float32(1e30)
TINY = np.float32(2.0 ** -60)
HUGE = np.float32(1e9)


def pair_order(nodes):
    """node index of every pair record: the inner nodes breadth-first from node 0, as uvrt_set_scene numbers them
    (none when the root is a leaf)"""
    left, count = nodes["leftFirst"], nodes["triCount"]
    order = [0] if count[0] == 0 else []
    qi = 0
    while qi < len(order):
        l = int(left[order[qi]])
        for ch in (l, l + 1):
            if count[ch] == 0:
                order.append(ch)
        qi += 1
    return np.array(order, dtype=np.int64)


def _leaf_ref(first, count):
    return REF_LEAF_BIT | (min(int(count), 15) << REF_COUNT_SHIFT) | int(first)


def _outside(v):
    """bounds the shortcuts' proofs do not cover: below 2^-60 (and not zero), above 1e9, infinite or NaN"""
    a = np.abs(v)
    return bool(np.any(((v != 0) & (a < TINY)) | ~(a <= HUGE)))


def layout(tris, nodes, tri_idx):
    """dict: pairs uint32[P, 16], quads uint32[Q, 32], leaf_count uint32[T], root_ref, top_pairs, top_quads, force_exact"""
    T = tris.shape[0]
    left, count = nodes["leftFirst"].astype(np.int64), nodes["triCount"].astype(np.int64)
    order = pair_order(nodes)
    P = order.size
    index = np.full(len(nodes), -1, dtype=np.int64)        # node -> pair
    index[order] = np.arange(P)
    # the two children of every pair, [P, 2]
    kids = left[order][:, None] + np.arange(2)[None, :] if P else np.zeros((0, 2), dtype=np.int64)
    leaf = count[kids] > 0
    refs = np.where(leaf, REF_LEAF_BIT | (np.minimum(count[kids], 15) << REF_COUNT_SHIFT) | left[kids], index[kids]).astype(np.uint32)
    leaf_count = np.zeros(T, dtype=np.uint32)
    leaf_count[left[kids][leaf]] = count[kids][leaf]
    root_ref = 0
    if count[0] > 0:
        root_ref = _leaf_ref(left[0], count[0])
        leaf_count[left[0]] = count[0]
    box = np.stack([nodes[k] for k in ("minx", "miny", "minz", "maxx", "maxy", "maxz")], axis=-1).astype(np.float32)   # [N, 6]
    kb = box[kids].view(np.uint32)                          # [P, 2, 6]
    pairs = np.zeros((P, 16), dtype=np.uint32)
    pairs[:, 0:3], pairs[:, 3] = kb[:, 0, 0:3], refs[:, 0]
    pairs[:, 4:7], pairs[:, 7] = kb[:, 0, 3:6], refs[:, 1]
    pairs[:, 8:11], pairs[:, 12:15] = kb[:, 1, 0:3], kb[:, 1, 3:6]
    depth = np.zeros(P, dtype=np.int64)
    for i in range(P):                                      # breadth-first: a parent comes before its children
        for k in (0, 1):
            if not leaf[i, k]:
                depth[refs[i, k]] = depth[i] + 1
    top_pairs = min(int((depth < 8).sum()), TOP6_MAX)       # depths never fall along the order: a prefix

    # the 4-wide collapse: a node's children are its pair's leaves and its pair's inner children's children
    qpair, qdepth, quads = ([0], [0], []) if P else ([], [], [])
    qi = 0
    while qi < len(qpair):
        ch = []                                             # (box of 6 words, ref)
        for k in (0, 1):
            p = qpair[qi]
            if leaf[p, k]:
                ch.append((kb[p, k], int(refs[p, k])))
            else:
                g = int(refs[p, k])
                ch += [(kb[g, j], int(refs[g, j])) for j in (0, 1)]
        q = np.zeros(32, dtype=np.uint32)
        far = FAR_BOX.view(np.uint32)
        for k in range(4):
            if k < len(ch):
                b, r = ch[k]
                if r < REF_LEAF_BIT:
                    qpair.append(r)
                    qdepth.append(qdepth[qi] + 1)
                    r = 2 * (len(qpair) - 1)
                q[4 * k:4 * k + 4] = (b[0], b[3], b[2], b[5])           # min.x, max.x, min.z, max.z
                q[16 + 2 * k:16 + 2 * k + 2] = (b[1], b[4])             # min.y, max.y
                q[24 + k] = r
            else:
                q[4 * k:4 * k + 4] = far
                q[16 + 2 * k:16 + 2 * k + 2] = far
                q[24 + k] = REF_DONE
        quads.append(q)
        qi += 1
    top_quads = min(sum(1 for d in qdepth if d < 4), TOP_QUADS_MAX)

    vertices = tris[:, [0, 1, 2, 4, 5, 6, 8, 9, 10]]        # the fourth component of a vertex is padding
    force_exact = _outside(box[kids.reshape(-1)]) or not bool(np.all(np.abs(vertices) <= HUGE))
    return {"pairs": pairs, "quads": np.array(quads, dtype=np.uint32).reshape(len(quads), 32), "leaf_count": leaf_count,
            "root_ref": root_ref, "top_pairs": top_pairs, "top_quads": top_quads, "force_exact": bool(force_exact)}

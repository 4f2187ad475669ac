"""A restatement of the face-resolved bounces with a reflectance per face (include/uvrt.h "per-face reflectance") in
numpy f64, one rounding per operator, with explicit loops over the samples, the faces and the bounces, in order: the rule of
uvrt_gather_indirect_linked_mapped on top of gather_faces_restate (its irradiance, sided links and hand-made scenes).  Also the
rules file of RayTracer::reflectMap, line by line.
Shared by tests/test_gather_reflect_map_cpu.py, tests/test_gpu_gather_reflect_map.py and tests/tools/gather_reflect_map_quality.py."""
import numpy as np

import gather_faces_restate as gf
import gather_links_restate as gl
import gather_restate as gr

f32 = np.float32


def as_planes(rho, T):
    """rho as f32[2][T]: a scalar fills both planes"""
    r = np.asarray(rho, dtype=f32)
    return np.broadcast_to(r, (2, T)).copy() if r.ndim == 0 else r.reshape(2, T)


def radiosity(rho, e):
    """r[f][h] = (double)rho[f][h] * e[f][h]: what face f of h sends back"""
    return np.asarray(rho, dtype=f32).astype(np.float64) * e


def bounce(nn, r, links):
    """g[2][T] from the radiosity r[2][T] and the sided links of all T triangles: sample s leaves face s & 1; no reflectance on
    the receiver"""
    links = np.asarray(links, dtype=np.int64)
    T, S2 = links.shape
    g = np.zeros((2, T), dtype=np.float64)
    with np.errstate(all="ignore"):
        for f in (0, 1):
            tot = np.zeros(T, dtype=np.float64)
            for s in range(f, S2, 2):
                L = links[:, s]
                Lc = np.clip(L, 0, None)
                tot = tot + np.where(L >= 0, r[Lc & 1, Lc >> 1], 0.0)
            gf_ = (0.5 * nn) * ((2.0 * tot) / np.float64(S2))
            g[f] = np.where(nn == 0.0, 0.0, gf_)
    return g


def bounces(tris, faces, links, rho, K):
    """([g_1, .., g_K], [e_0, .., e_K]), each f64[2][T]; rho f32[2][T] or a scalar"""
    nn = gl.normals(tris)
    links = np.asarray(links).reshape(nn.size, -1)
    rho = as_planes(rho, nn.size)
    e = [gf.irradiance(nn, faces)]
    g = []
    for _ in range(K):
        g.append(bounce(nn, radiosity(rho, e[-1]), links))
        e.append(gf.irradiance(nn, g[-1]))
    return g, e


def linked(tris, faces, links, rho, K, first=0, count=None, base=None):
    """expected[first, first + count) of uvrt_gather_indirect_linked_mapped; with `base` (add = 1, f64[count]) base + total"""
    T = tris.shape[0]
    count = T - first if count is None else count
    g, _ = bounces(tris, faces, links, rho, K)
    total = g[0][0] + g[0][1]
    for b in range(1, K):
        total = total + (g[b][0] + g[b][1])
    total = total[first:first + count]
    return total if base is None else np.asarray(base, dtype=np.float64) + total


def bound(K, S2):
    """|mapped / sided - 1| at a constant rho: K * (S2 + 16) * 2^-53 (include/uvrt.h)"""
    return K * (S2 + 16) * 2.0 ** -53


# ---------------------------------------------------------------- the rules file
class RulesError(ValueError):
    pass


def parse_rules(text, name="rules"):
    """[(lo f32[3], hi f32[3], rho f32, toward f32[3] or None)], in file order; RulesError names the file and the line"""
    rules = []
    for no, line in enumerate(text.splitlines(), 1):
        words = line.split("#", 1)[0].split()
        if not words:
            continue

        def bad(why):
            return RulesError("%s:%d: %s" % (name, no, why))
        if words[0] != "box":
            raise bad("unknown keyword '%s'" % words[0])
        if len(words) == 8:
            nums, toward = words[1:8], None
        elif len(words) == 12 and words[8] == "toward":
            nums, toward = words[1:8], words[9:12]
        else:
            raise bad("box takes X0 Y0 Z0 X1 Y1 Z1 RHO [toward PX PY PZ]")
        try:
            with np.errstate(over="ignore"):
                v = [f32(float(w)) for w in nums]
                p = None if toward is None else np.array([f32(float(w)) for w in toward], dtype=f32)
        except ValueError:
            raise bad("not a number")
        if np.any(np.isnan(v)) or (p is not None and not np.all(np.isfinite(p))):     # (a box may reach to infinity)
            raise bad("not a finite number")
        if not np.isfinite(v[6]) or not (f32(0.0) <= v[6] <= f32(1.0)):
            raise bad("RHO must be finite and in [0, 1]")
        lo, hi = np.array(v[0:3], dtype=f32), np.array(v[3:6], dtype=f32)
        if np.any(lo > hi):
            raise bad("a lower bound of the box lies above its upper bound")
        rules.append((lo, hi, v[6], p))
    return rules


def apply_rules(tris, rules, base):
    """rho f32[2][T]: every entry starts at `base`; later rules override earlier ones.  A box holds the triangles whose stored
    centroid (tris[:, 12:15]) lies in it, bounds included, compared in f32.  `toward P`: only the face that looks at P -- face 0
    iff n.(P - v0) > 0 with n = cross(e1, e2), all in f64 from the f32 values; a triangle with nn == 0 is left as it is"""
    tris = np.ascontiguousarray(tris, dtype=f32)
    T = tris.shape[0]
    rho = np.full((2, T), f32(base), dtype=f32)
    cen = tris[:, 12:15]
    _, _, n, nn = gr.tri_normals(tris)
    v0 = tris[:, 0:3].astype(np.float64)
    for lo, hi, value, p in rules:
        inside = np.all((cen >= lo[None, :]) & (cen <= hi[None, :]), axis=1)
        if p is None:
            rho[:, inside] = value
            continue
        d = p.astype(np.float64)[None, :] - v0
        with np.errstate(all="ignore"):
            c = (n[:, 0] * d[:, 0] + n[:, 1] * d[:, 1]) + n[:, 2] * d[:, 2]
        face = np.where(c > 0.0, 0, 1)
        hit = inside & (nn != 0.0)
        idx = np.nonzero(hit)[0]
        rho[face[idx], idx] = value
    return rho


def rules_map(tris, text, base, name="rules"):
    return apply_rules(tris, parse_rules(text, name), base)

"""A restatement of the virtual dosimeters (include/uvrt.h "sensors") in numpy f32 / f64, one rounding per operator: the samples
of uvrt_gather_sensors, their weights, the reduction and its variance; the rays of uvrt_gather_sensors_indirect, the look-up
at their closest hits and the reduction; uvrt_accumulate_sensors and uvrt_sensor_dosage.  The RNG, the occlusion query and the
triangle normals are gather_restate's, the closest hit is gather_indirect_restate's (both orc.extend with `dist` preset).
Shared by tests/test_gather_sensors_cpu.py and tests/test_gpu_gather_sensors.py."""
import numpy as np

import gather_indirect_restate as gir
import gather_restate as gr

f32 = np.float32
f64 = np.float64
u32 = np.uint32
PLANAR, SPHERICAL = 0, 1
SENSOR_DT = np.dtype([("pos", "<f4", (3,)), ("normal", "<f4", (3,)), ("kind", "<i4"), ("reserved", "<i4")])
GOLDEN = u32(0x9E3779B9)


def sensors(rows):
    """SENSOR_DT records from (pos, normal or None) rows: a row without a normal is spherical"""
    out = np.zeros(len(rows), dtype=SENSOR_DT)
    for k, (pos, normal) in enumerate(rows):
        out[k]["pos"] = pos
        out[k]["kind"] = SPHERICAL if normal is None else PLANAR
        if normal is not None:
            out[k]["normal"] = normal
    return out


ROOM_LO, ROOM_HI = (-1.68, -1.44, -3.73), (1.63, 1.31, 5.56)      # the box bench.soup_triangles fills


def edge_sensors(scene, K, lamp=(0.0, 0.0, 0.0), seed=5):
    """K sensors for the edge scene of tests/gather_edge_scene.py, generated from a seed: points in the soup's box with random
    normals, every third one spherical, and hand-made ones at the end, as many as fit (the last first): one on a triangle's
    surface facing along its normal; one at the lamp's foot (r = 0 at light_length 0); one at x = 3e19, where d.x * d.x
    overflows f32 while D stays finite; one whose normal ties on two zero components; one whose normal ties on all three"""
    rng = np.random.default_rng(seed)
    out = np.zeros(K, dtype=SENSOR_DT)
    out["pos"] = rng.uniform(ROOM_LO, ROOM_HI, (K, 3)).astype(f32)
    out["normal"] = rng.normal(size=(K, 3)).astype(f32)
    out["kind"] = np.where(np.arange(K) % 3 == 1, SPHERICAL, PLANAR)
    tri = np.asarray(scene.tris[3], dtype=f32)
    v0, v1, v2 = tri[0:3], tri[4:7], tri[8:11]
    centre = ((v0 + v1) + v2) / f32(3.0)
    n_tri = np.cross((v1 - v0).astype(f64), (v2 - v0).astype(f64)).astype(f32)
    hand = ((centre, n_tri, PLANAR), (lamp, (0.0, 1.0, 0.0), PLANAR), ((3e19, 0.0, 0.0), (-1.0, 0.0, 0.0), PLANAR),
            ((0.5, 0.25, -0.5), (0.0, 0.0, -2.0), PLANAR), ((-0.5, 0.75, 1.0), (1.0, 1.0, 1.0), PLANAR),
            (lamp, (0.0, 0.0, 0.0), SPHERICAL), ((3e19, 0.0, 0.0), (0.0, 0.0, 0.0), SPHERICAL))
    for i, (pos, normal, kind) in enumerate(hand):
        if i < K:
            out[K - 1 - i] = (tuple(pos), tuple(normal), kind, 0)
    return out


def _index(first, count, S):
    k = np.repeat(np.arange(first, first + count, dtype=np.uint64), S)
    s = np.tile(np.arange(S, dtype=np.uint64), count)
    j = ((k * np.uint64(S) + s) & np.uint64(0xFFFFFFFF)).astype(u32)
    return k.astype(u32), s.astype(u32), j


def samples(orc, sens, frm, to, length, S, seed, mode=0, first=0, count=None):
    """The direct samples of sensors [first, first + count): (rays RAY_DT[count * S] with dist = tmax, w f64[count * S])"""
    count = len(sens) - first if count is None else count
    k, s, j = _index(first, count, S)
    rng = gr.wang_hash(j ^ gr.wang_hash(u32(seed)))
    u_h, rng = gr.random_float(rng)
    u_m, rng = gr.random_float(rng)
    if mode == 1:
        u_h = (s.astype(f32) + u_h) / f32(S)
        assert u_h.dtype == f32
        with np.errstate(over="ignore"):
            h_k = gr.wang_hash(k ^ gr.wang_hash(u32(seed) ^ GOLDEN))
            m = s * GOLDEN + h_k
        u_m = (m >> u32(8)).astype(f32) * f32(5.9604644775390625e-8)
    loc = np.repeat(np.arange(first, first + count), S)
    p = np.ascontiguousarray(sens["pos"][loc], dtype=f32)
    n = np.ascontiguousarray(sens["normal"][loc], dtype=f32).astype(f64)
    kind = sens["kind"][loc]
    fr = [f32(v) for v in frm]
    sg = [f32(f32(x) - f32(v)) for x, v in zip(to, frm)]
    ox = fr[0] + u_m * sg[0]
    oy = (fr[1] + u_h * f32(length)) + u_m * sg[1]
    oz = fr[2] + u_m * sg[2]
    with np.errstate(all="ignore"):
        dx, dy, dz = p[:, 0] - ox, p[:, 1] - oy, p[:, 2] - oz
        r = np.sqrt((dx * dx + dy * dy) + dz * dz)
        assert r.dtype == f32
        D = np.stack([dx, dy, dz], axis=1).astype(f64)
        R2 = (D[:, 0] * D[:, 0] + D[:, 1] * D[:, 1]) + D[:, 2] * D[:, 2]
        R = np.sqrt(R2)
        nn = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        c = (n[:, 0] * D[:, 0] + n[:, 1] * D[:, 1]) + n[:, 2] * D[:, 2]
        w_planar = np.where(c < 0.0, (-c) / ((nn * (R2 * R)) * gr.FOUR_PI), 0.0)
        w_sphere = 1.0 / (R2 * gr.FOUR_PI)
        w = np.where(kind == PLANAR, w_planar, w_sphere)
        traced = np.isfinite(r) & (r > 0) & (w > 0.0)       # a sample that weighs 0 is not traced
        rays = np.zeros(count * S, dtype=orc.RAY_DT)
        rays["dirx"], rays["diry"], rays["dirz"] = dx / r, dy / r, dz / r
        rays["dist"] = r * gr.TMAX_FACTOR
    rays["origx"], rays["origy"], rays["origz"] = ox, oy, oz
    for f, v in (("dirx", 0.0), ("diry", 1.0), ("dirz", 0.0), ("dist", 0.0)):
        rays[f][~traced] = f32(v)
    w = np.where(traced, w, 0.0)
    return rays, w


def reduce(w, occ, S, photons_equiv, mode=0):
    """(density, variance) f64[count] from the samples' weights and occlusion bytes"""
    x = np.where(occ.reshape(-1, S) != 0, 0.0, w.reshape(-1, S))
    count = x.shape[0]
    total = np.zeros(count, dtype=f64)
    for s in range(S):
        total = total + x[:, s]
    c = f64(photons_equiv)
    m = total / f64(S)
    density = c * m
    variance = np.zeros(count, dtype=f64)
    if S >= 2:
        q = np.zeros(count, dtype=f64)
        if mode == 0:
            for s in range(S):
                d = x[:, s] - m
                q = q + d * d
        else:
            for s in range(1, S):
                d = x[:, s] - x[:, s - 1]
                q = q + d * d
        SS = f64(S) * f64(S - 1)
        v = q / SS if mode == 0 else q / (2.0 * SS)
        variance = (c * c) * v
    return density, variance


def gather(orc, scene, sens, frm, to, length, S, seed, photons_equiv, mode=0, flavour=0, first=0, count=None):
    """(density, variance, rays, occluded) of uvrt_gather_sensors"""
    rays, w = samples(orc, sens, frm, to, length, S, seed, mode, first, count)
    occ = gr.occluded(orc, scene, rays, flavour)
    density, variance = reduce(w, occ, S, photons_equiv, mode)
    return density, variance, rays, occ


def indirect_rays(orc, sens, S, seed, first=0, count=None):
    """The reflected rays of sensors [first, first + count): RAY_DT[count * S] with dist = tmax"""
    count = len(sens) - first if count is None else count
    _, _, j = _index(first, count, S)
    rng = gr.wang_hash(j ^ gr.wang_hash(u32(seed)))
    x = np.zeros(count * S)
    y = np.zeros(count * S)
    done = np.zeros(count * S, dtype=bool)
    for _ in range(gir.ROUNDS):
        xf, rng = gr.random_float(rng)
        yf, rng = gr.random_float(rng)
        xd = (xf * f32(2.0) - f32(1.0)).astype(f64)
        yd = (yf * f32(2.0) - f32(1.0)).astype(f64)
        take = ~done & ((xd * xd + yd * yd) <= 1.0)
        x[take], y[take] = xd[take], yd[take]
        done |= take
    loc = np.repeat(np.arange(first, first + count), S)
    p = np.ascontiguousarray(sens["pos"][loc], dtype=f32)
    n = np.ascontiguousarray(sens["normal"][loc], dtype=f32).astype(f64)
    kind = sens["kind"][loc]
    q = x * x + y * y
    with np.errstate(all="ignore"):
        z = np.sqrt(1.0 - q)
        nn = np.sqrt((n[:, 0] * n[:, 0] + n[:, 1] * n[:, 1]) + n[:, 2] * n[:, 2])
        a = np.abs(n)
        ax_x = (a[:, 0] <= a[:, 1]) & (a[:, 0] <= a[:, 2])
        ax_y = ~ax_x & (a[:, 1] <= a[:, 2])
        zero = np.zeros(count * S)
        Cx = np.where(ax_x, zero, np.where(ax_y, n[:, 2], -n[:, 1]))
        Cy = np.where(ax_x, -n[:, 2], np.where(ax_y, zero, n[:, 0]))
        Cz = np.where(ax_x, n[:, 1], np.where(ax_y, -n[:, 0], zero))
        cl = np.sqrt((Cx * Cx + Cy * Cy) + Cz * Cz)
        Tx, Ty, Tz = Cx / cl, Cy / cl, Cz / cl
        Bx = (n[:, 1] * Tz - n[:, 2] * Ty) / nn
        By = (n[:, 2] * Tx - n[:, 0] * Tz) / nn
        Bz = (n[:, 0] * Ty - n[:, 1] * Tx) / nn
        zz = z / nn
        Px = ((x * Tx) + (y * Bx)) + (zz * n[:, 0])
        Py = ((x * Ty) + (y * By)) + (zz * n[:, 1])
        Pz = ((x * Tz) + (y * Bz)) + (zz * n[:, 2])
        g = np.sqrt(1.0 - q)
        Sx, Sy, Sz = (2.0 * x) * g, (2.0 * y) * g, 1.0 - 2.0 * q
        planar = kind == PLANAR
        d = np.stack([np.where(planar, Px, Sx), np.where(planar, Py, Sy), np.where(planar, Pz, Sz)], axis=1).astype(f32)
    traced = (~planar | (nn != 0.0)) & np.isfinite(d).all(axis=1) & (d != 0).any(axis=1)
    out = np.zeros(count * S, dtype=orc.RAY_DT)
    out["dirx"] = np.where(traced, d[:, 0], f32(0))
    out["diry"] = np.where(traced, d[:, 1], f32(1))
    out["dirz"] = np.where(traced, d[:, 2], f32(0))
    out["origx"], out["origy"], out["origz"] = p[:, 0], p[:, 1], p[:, 2]
    out["dist"] = np.where(traced, gir.MISS, f32(0.0))
    return out


def indirect_reduce(tris, sens, rays, h, S, rho, emitter, source=None, faces=None, rho_map=None, first=0, count=None):
    """the reflected part f64[count] of sensors [first, first + count) from the hit triangles h (-1: a miss): what the call
    adds to density.  emitter 0: `source` f64[T] under rho; emitter 1: `faces` f64[2][T] under rho or rho_map f32[2][T]"""
    count = len(sens) - first if count is None else count
    T = tris.shape[0]
    _, _, n_all, nn_all = gr.tri_normals(np.ascontiguousarray(tris, dtype=f32))
    h = np.asarray(h, dtype=np.int64)
    hc = np.clip(h, 0, T - 1)
    ok = (h >= 0) & (nn_all[hc] > 0)
    with np.errstate(all="ignore"):
        if emitter == 0:
            y = f64(f32(rho)) * (np.asarray(source, dtype=f64)[hc] / (0.5 * nn_all[hc]))
        else:
            nh = n_all[hc]
            d = np.stack([rays["dirx"], rays["diry"], rays["dirz"]], axis=1).astype(f64)
            c = (nh[:, 0] * d[:, 0] + nh[:, 1] * d[:, 1]) + nh[:, 2] * d[:, 2]
            a = np.where(c < 0.0, 0, 1)
            fa = np.asarray(faces, dtype=f64).reshape(2, T)[a, hc]
            ra = f64(f32(rho)) if rho_map is None else np.asarray(rho_map, dtype=f32).reshape(2, T)[a, hc].astype(f64)
            y = ra * (fa / (0.5 * nn_all[hc]))
        y = np.where(ok, y, 0.0).reshape(count, S)
        tot = np.zeros(count, dtype=f64)
        for s in range(S):
            tot = tot + y[:, s]
        kind = sens["kind"][first:first + count]
        return np.where(kind == PLANAR, tot / f64(S), (4.0 * tot) / f64(S))


def indirect(orc, scene, sens, S, seed, rho, emitter, source=None, faces=None, rho_map=None, flavour=0, first=0, count=None):
    """(what uvrt_gather_sensors_indirect adds to density f64[count], rays, hit triangles)"""
    r = indirect_rays(orc, sens, S, seed, first, count)
    _, h = gir.closest(orc, scene, r, flavour)
    return indirect_reduce(scene.tris, sens, r, h, S, rho, emitter, source, faces, rho_map, first, count), r, h


def accumulate(planes, time_step):
    """uvrt_accumulate_sensors on planes f64[5][K] (density, variance, dose_map, max_map, var_map), in place"""
    dt = f64(f32(time_step))
    planes[2] = planes[2] + planes[0] * dt
    planes[3] = np.where(planes[3] < planes[0], planes[0], planes[3])
    planes[4] = planes[4] + planes[1] * (dt * dt)
    planes[0] = 0.0
    planes[1] = 0.0


def dosage(map_, photons_per_light, scaled_power):
    """uvrt_sensor_dosage: k_compute_dosage's arithmetic with area = 1.0f"""
    den = f32(1.0) * f32(photons_per_light)
    return ((f64(f32(scaled_power)) * np.asarray(map_, dtype=f64)) / f64(den)).astype(f32)


# ---------------------------------------------------------------- the rules file (RayTracer::ParseSensorRules)
class RulesError(ValueError):
    pass


def _number(word):
    """a whole word as a finite number, rounded once to f32 (strtod's forms: no underscores, no surrounding blanks)"""
    try:
        if "_" in word or word != word.strip():
            raise ValueError
        v = float.fromhex(word) if word.lower().lstrip("+-").startswith("0x") else float(word)
    except ValueError:
        return None
    with np.errstate(over="ignore"):
        v = f32(v)
    return v if np.isfinite(v) else None


def rules_sensors(text, name="sensors.rules"):
    """SENSOR_DT records of a rules file's text, in file order; RulesError("NAME:LINE: reason") for a line that cannot be read"""
    out = []
    for no, line in enumerate(text.split("\n"), 1):
        w = line.split("#", 1)[0].split()
        if not w:
            continue

        def bad(why):
            return RulesError("%s:%d: %s" % (name, no, why))
        if w[0] not in ("sensor", "grid"):
            raise bad("unknown keyword '%s'" % w[0])
        grid = w[0] == "grid"
        at = 10 if grid else 4
        form = "grid takes X0 Y0 Z0 X1 Y1 Z1 NX NY NZ sphere | planar MX MY MZ" if grid else "sensor takes X Y Z sphere | planar NX NY NZ"
        if len(w) <= at:
            raise bad(form)
        if w[at] not in ("planar", "sphere"):
            raise bad("unknown kind '%s' (planar or sphere)" % w[at])
        planar = w[at] == "planar"
        if len(w) != at + (4 if planar else 1):
            raise bad(form)
        v = []
        for word in w[1:7 if grid else 4] + (w[at + 1:at + 4] if planar else []):
            x = _number(word)
            if x is None:
                raise bad("'%s' is not a finite number" % word)
            v.append(x)
        n = v[-3:] if planar else [f32(0)] * 3
        if planar and all(x == 0 for x in n):
            raise bad("a planar sensor's normal is zero")
        cells = [1, 1, 1]
        for k in range(3 if grid else 0):
            word = w[7 + k]
            digits = word[1:] if word[:1] in "+-" else word
            if not digits.isdigit() or not digits.isascii() or not 1 <= int(word) <= 1 << 24:
                raise bad("'%s' is not an integer >= 1" % word)
            cells[k] = int(word)
        if len(out) + cells[0] * cells[1] * cells[2] > 1 << 24:
            raise bad("more than %d sensors" % (1 << 24))
        kind = PLANAR if planar else SPHERICAL
        if not grid:
            out.append((tuple(v[:3]), tuple(n), kind, 0))
            continue
        axis = [v[a] + (v[3 + a] - v[a]) * ((np.arange(cells[a], dtype=f32) + f32(0.5)) / f32(cells[a])) for a in range(3)]
        assert all(a.dtype == f32 for a in axis)
        for z in axis[2]:
            for y in axis[1]:
                for x in axis[0]:
                    out.append(((x, y, z), tuple(n), kind, 0))
    return np.array(out, dtype=SENSOR_DT) if out else np.zeros(0, dtype=SENSOR_DT)

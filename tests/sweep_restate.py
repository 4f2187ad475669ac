"""A restatement of uvrt_generate_sweep (include/uvrt.h) from the oracle library's pieces: orc_generate_one gives work-item
gid's ray at `from` and its RNG state afterwards, orc_random_float the next draw u, numpy f32 the three interpolations
fl(a + fl(u * fl(b - a))).  Shared by tests/test_free_cpu.py and tests/test_gpu_sweep.py."""
import ctypes as C

import numpy as np

f32 = np.float32


def _lib(orc):
    L = orc.lib()
    L.orc_random_float.restype = C.c_float
    L.orc_random_float.argtypes = [C.POINTER(C.c_uint32)]
    return L


def _one(L, orc, ray, gid, frm3, length, SEED):
    """work-item gid reading SEED: fills ray[0] (generate.cl's), returns (u, RNG state after the draw of u)"""
    s = C.c_uint32(L.orc_generate_one(ray.ctypes.data_as(C.c_void_p), int(gid), frm3, float(f32(length)), int(SEED)))
    u = L.orc_random_float(C.byref(s))
    return f32(u), int(s.value)


def seed_next_sweep(orc, frm, length, seed_prev):
    L = _lib(orc)
    ray = np.zeros(1, dtype=orc.RAY_DT)
    return _one(L, orc, ray, 0, orc._f3(frm), length, seed_prev)[1]


def sweep(orc, first, n, frm, to, length, SEED):
    """(rays[n] for global ids [first, first + n), SEED_k): mode-0 SEED semantics -- work-item 0 reads SEED_{k-1}, every
    other work-item SEED_k = work-item 0's state after its draw of u"""
    L = _lib(orc)
    frm3 = orc._f3(frm)
    nxt = seed_next_sweep(orc, frm, length, SEED)
    rays = np.zeros(n, dtype=orc.RAY_DT)
    u = np.zeros(n, dtype=np.float32)
    one = np.zeros(1, dtype=orc.RAY_DT)
    for i in range(n):
        gid = first + i
        u[i], _ = _one(L, orc, one, gid, frm3, length, SEED if gid == 0 else nxt)
        rays[i] = one[0]
    a = [f32(v) for v in frm]
    d = [f32(f32(t) - f32(v)) for t, v in zip(to, frm)]
    assert np.array_equal(rays["origx"], np.full(n, a[0])) and np.array_equal(rays["origz"], np.full(n, a[2]))
    rays["origx"] = a[0] + u * d[0]
    rays["origy"] = rays["origy"] + u * d[1]          # generate's from.y + r1 * length, then the place on the segment
    rays["origz"] = a[2] + u * d[2]
    assert rays["origx"].dtype == np.float32
    return rays, nxt


def segment_duration(a, b, speed):
    """len / driveSpeed as RayTracer::ComputeSegmentDosageMap forms it: strict f32, len = sqrtf(dx*dx + dz*dz)"""
    dx, dz = f32(f32(b[0]) - f32(a[0])), f32(f32(b[1]) - f32(a[1]))
    ln = np.sqrt(f32(f32(dx * dx) + f32(dz * dz)))
    return f32(f32(ln) / f32(speed))

"""CPU: RayTracer::RouteLaunches (host.route_launches), the one list of a route's launches, against a numpy float32
restatement: every record, all 40 bytes, bit for bit."""
import ctypes
import subprocess

import numpy as np
import pytest

f32 = np.float32
FLOOR = f32(-1.39548361)                    # the test room's floorHeight (test_host_cpu.py)
Y = f32(FLOOR + f32(0.8))                   # the caller's single f32 sum floorHeight + lightHeight


@pytest.fixture(scope="module")
def host(pkg):
    from uvrt_amd import host
    host.lib()
    return host


def restate(host, lamps, y, v):
    """the stops, then iff v > 0 and L >= 2 the segments: np.sqrt(dx*dx + dz*dz) / v on float32 scalars"""
    lamps = [tuple(f32(c) for c in l) for l in lamps]
    L = len(lamps)
    out = []
    for i, (x, z, d) in enumerate(lamps):
        out.append(((x, y, z), (0, 0, 0), d, 0, i, 0))
    if v > 0 and L >= 2:                    # (NaN > 0 is False)
        for k in range(L - 1):
            a, b = lamps[k], lamps[k + 1]
            dx, dz = b[0] - a[0], b[1] - a[1]
            out.append(((a[0], y, a[1]), (b[0], y, b[1]), np.sqrt(dx * dx + dz * dz) / f32(v), 1, L + k, 0))
    return np.array(out, dtype=host.ROUTE_LAUNCH_DT)


def same_bytes(a, b):
    return a.dtype == b.dtype and a.tobytes() == b.tobytes()


def test_the_record_is_40_bytes(host, pkg):
    dt = host.ROUTE_LAUNCH_DT
    assert dt.itemsize == 40
    assert [dt.fields[f][1] for f in ("from", "to", "duration", "kind", "column")] == [0, 12, 24, 28, 32]
    assert (pkg.capi.LAUNCH_STOP, pkg.capi.LAUNCH_SWEEP) == (0, 1)


def test_lange_route_at_a_tenth_of_a_metre_per_second(host, oroute):
    lamps = oroute["lamps"]
    assert len(lamps) == 12
    got = host.route_launches(lamps, Y, 0.1)
    assert len(got) == 23 and list(got["column"]) == list(range(23))
    assert list(got["kind"]) == [0] * 12 + [1] * 11
    assert same_bytes(got, restate(host, lamps, Y, 0.1))
    assert (got["duration"][12:] > 0).all()


def test_a_repeated_position_makes_a_segment_of_duration_zero(host, oroute):
    lamps = [oroute["lamps"][k] for k in (0, 1, 1, 2)]
    got = host.route_launches(lamps, Y, 0.05)
    assert len(got) == 7
    assert same_bytes(got, restate(host, lamps, Y, 0.05))
    seg = got["duration"][4:]
    assert seg[1].tobytes() == f32(0.0).tobytes()           # +0.0, not -0.0
    assert seg[0] == f32(17.084578) and seg[2] == f32(12.022787)
    assert np.array_equal(got["from"][5], got["to"][5])


def test_one_position_has_no_segment(host, oroute):
    lamps = oroute["lamps"][:1]
    got = host.route_launches(lamps, Y, 0.1)
    assert len(got) == 1 and same_bytes(got, restate(host, lamps, Y, 0.1))


@pytest.mark.parametrize("speed", [0.0, -1.0, float("nan")])
def test_no_speed_means_the_stops_only(host, oroute, speed):
    lamps = oroute["lamps"]
    got = host.route_launches(lamps, Y, speed)
    assert len(got) == 12 and (got["kind"] == 0).all()
    assert same_bytes(got, restate(host, lamps, Y, speed))


def test_no_position_no_record(host):
    assert len(host.route_launches([], Y, 0.1)) == 0


def test_max_smaller_than_the_count(host, oroute):
    xzd = np.ascontiguousarray(oroute["lamps"], dtype=f32)
    out = np.full(23 * 40, 0xAB, dtype=np.uint8)
    n = host.lib().uvrt_host_route_launches(xzd.ctypes.data, 12, float(Y), 0.1, out.ctypes.data, 5)
    assert n == 23
    assert out[:200].tobytes() == restate(host, oroute["lamps"], Y, 0.1)[:5].tobytes()
    assert (out[200:] == 0xAB).all()
    assert host.lib().uvrt_host_route_launches(xzd.ctypes.data, 12, float(Y), 0.1, None, 0) == 23
    assert host.lib().uvrt_host_route_launches(xzd.ctypes.data, 12, float(Y), 0.1, out.ctypes.data, -1) == 23
    assert (out[200:] == 0xAB).all()


def test_the_symbol_is_bound_once_and_exported(host):
    assert [s[0] for s in host.SYMBOLS].count("uvrt_host_route_launches") == 1
    assert hasattr(ctypes.CDLL(host.LIB_PATH), "uvrt_host_route_launches")
    names = {l.split()[-1] for l in subprocess.check_output(["nm", "-D", "--defined-only", host.LIB_PATH], text=True).splitlines()}
    assert {n for n in names if n.startswith("uvrt_host_")} == {s[0] for s in host.SYMBOLS}

"""GPU: the virtual dosimeters against closed-form radiometry (tests/radiometry_sensors.py).  Nothing here is compared
with a restatement: the mean of density[k] over K = 8 seeds of S = 4096 samples is held against the rod's closed forms, a point
lamp's cos theta / 4 pi R^2, Lambert's form factors and solid angles, under the acceptance rule of DESIGN.md 24

    |mean over the K S samples - mu_ref| <= 6 sigma_ref / sqrt(K S) + eps_quad + 1e-5 mu_ref

and a reference of exactly 0 demands exactly +0.0 in every call.  tests/test_radiometry_sensors_cpu.py shows that each case would
notice each wrong formula.  The oracle library is used for the BVH alone.

With UVRT_RADIOMETRY_MARGINS=FILE the margins of every case are written into FILE under "gpu"."""
import numpy as np
import pytest

import gather_edge_scene as ge
import radiometry_scenes as rs
import radiometry_sensors as rx

pytestmark = pytest.mark.gpu

N, K, S, SEEDS = rx.N, rx.K, rx.S, rx.SEEDS
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _margins():
    yield
    rs.dump_margins("gpu")


def new_ctx(pkg, orc, rows, sensors, fl=0, mode=0):
    scene = ge.HandScene(orc, np.array(rows, dtype=f32))
    c = pkg.capi.Ctx(0)
    c.set_scene(scene.tris, scene.nodes, scene.triIdx)
    c.resize_rays(len(sensors) * S)
    c.set_flavour(fl)
    c.set_gather_sampling(mode)
    c.set_sensors([pkg.capi.sensor(p, n) for p, n in sensors])
    return c


def done(c):
    c.sync()
    c.close()


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", tuple(rx.DIRECT_CASES))
def test_the_rod(pkg, orc, name, mode, fl):
    """planar and spherical sensors beside, below, above and on the axis of a 1.2 m rod, at a stop and on a sweep"""
    _, frm, to, length = rx.DIRECT_CASES[name]
    c = new_ctx(pkg, orc, rx.direct_rows(name), rx.ROD_SENSORS, fl, mode)
    got = []
    for seed in SEEDS:
        c.gather_sensors(frm, to, length, S, seed, N)
        got.append(c.read_sensor_plane(0))
    done(c)
    rs.accept("sensors, %s, mode %d, flavour %d" % (name, mode, fl), np.mean(got, axis=0), rx.direct_reference(name), K * S)


@pytest.mark.parametrize("fl", (0, 1))
def test_the_point_lamp_and_the_plate(pkg, orc, fl):
    """in the light N cos theta / 4 pi R^2; in the plate's shadow and facing away exactly +0.0 in every call"""
    ref = rx.plate_reference()
    c = new_ctx(pkg, orc, rs.floor_rows(True), rx.PLATE_SENSORS, fl)
    got = []
    for seed in SEEDS:
        c.gather_sensors(rs.LAMP, rs.LAMP, 0.0, S, seed, N)
        got.append(c.read_sensor_plane(0))
    done(c)
    got = np.array(got)
    rs.accept("sensors, point lamp, plate, flavour %d" % fl, got.mean(axis=0), ref, K * S)
    dark = ref["mu"] == 0
    assert dark.sum() == 3 and np.all(got[:, dark] == 0.0) and not np.signbit(got[:, dark]).any()


@pytest.mark.parametrize("fl", (0, 1))
@pytest.mark.parametrize("call", rx.BOUNCE_CALLS)
def test_the_reflected_part(pkg, orc, call, fl):
    """between the facing squares: a planar sensor against form factor times radiosity, a spherical one against (B / pi) Omega; with
    the face planes the light on the outer faces must not arrive, with the map every emitting face has its own rho"""
    source, faces, rho = rx.bounce_inputs(call)
    c = new_ctx(pkg, orc, rs.squares_rows(), rx.BOUNCE_SENSORS, fl)
    if source is not None:
        c.write_indirect_source(source)
    if faces is not None:
        c.write_gather_faces(0, faces[0])
        c.write_gather_faces(1, faces[1])
    if rho is not None:
        c.write_reflectance(0, rho[0])
        c.write_reflectance(1, rho[1])
    got = []
    for seed in SEEDS:
        c.reset_sensors()
        c.gather_sensors_indirect(rs.BOUNCE_RHO, S, seed, 0 if call == "source" else 1, 1 if call == "mapped" else 0)
        got.append(c.read_sensor_plane(0))
    done(c)
    rs.accept("sensors, reflected, %s, flavour %d" % (call, fl), np.mean(got, axis=0), rx.bounce_reference(call), K * S)


@pytest.mark.parametrize("mode", (0, 1))
def test_the_calibration_in_the_room(pkg, orc, mode):
    """RayTracer::CalibratePowerAtSensor on the sensor that faces the rod: the calibrated power against 0.01 P / closed form.  The
    calibrating launch is one call of CALIBRATION_SAMPLES samples with seed 0, so the rule holds it with that many samples"""
    from uvrt_amd import host
    ref = rx.calibration_reference()
    mesh = host.Mesh(tris=rx.direct_rows("rod"))
    rt = host.RayTracer(mesh=mesh, device=0)
    rt.set_lamps([(rs.ROD_FOOT[0], rs.ROD_FOOT[2], 1.0)])
    rt.lightHeight = rs.ROD_FOOT[1] - mesh.floorHeight
    assert f32(f32(mesh.floorHeight) + f32(rt.lightHeight)) == f32(rs.ROD_FOOT[1]), "the lamp's foot is the reference's"
    rt.lightLength = rs.ROD
    rt.photonCount = N
    rt.gatherSampling = mode
    rt.sensorSamples = rx.CALIBRATION_SAMPLES
    rt.set_sensors([pkg.capi.sensor(p, n) for p, n in rx.ROD_SENSORS])
    rt.ResetDosageMap()
    before = rt.ctx.read_photon_map(0).copy()
    power = rt.calibrate_power_at_sensor(rx.CALIBRATION_POWER, 0, 0)
    assert power == rt.lightIntensity == rt.calibratedPower and rt.sensorLaunches == 0
    assert np.all(np.stack([rt.ctx.read_sensor_plane(w) for w in range(5)]) == 0.0), "the sensor maps are reset again"
    assert np.array_equal(rt.ctx.read_photon_map(0), before) and rt.ctx.T == mesh.triangleCount, "neither the scene nor the triangle maps"
    rt.close()
    rs.accept("sensors, calibration, mode %d" % mode, np.array([power]), ref, rx.CALIBRATION_SAMPLES)

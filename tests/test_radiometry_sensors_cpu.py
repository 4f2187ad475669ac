"""CPU: the sensors' radiometry references (tests/radiometry_sensors.py) checked against themselves, the restatement
(tests/gather_sensors_restate.py) run through the same cases under the acceptance rule of DESIGN.md 24, and the power of every
case: each wrong formula that applies lies at least 3 tolerances off.

With UVRT_RADIOMETRY_MARGINS=FILE the margins of every case are written into FILE under "cpu"."""
import numpy as np
import pytest

import gather_edge_scene as ge
import gather_sensors_restate as gsr
import radiometry_reference as rr
import radiometry_scenes as rs
import radiometry_sensors as rx

N, K, S, SEEDS = rx.N, rx.K, rx.S, rx.SEEDS
f32 = np.float32


@pytest.fixture(scope="module", autouse=True)
def _margins():
    yield
    rs.dump_margins("cpu")


def records(sensors):
    return gsr.sensors(sensors)


def tolerance(ref, samples=K * S):
    return rr.tolerance(ref["sigma"], ref["eps"], ref["mu"], samples)


# ---------------------------------------------------------------- the references themselves
def test_the_closed_forms_agree_with_the_quadrature():
    for k in rx.CLOSED_FORM:
        sensor = rx.ROD_SENSORS[k]
        closed = rx.rod_closed_form(sensor, rs.ROD_FOOT, rs.ROD)
        quad, _, eps = rx.direct_moments(sensor, rs.ROD_FOOT, rs.ROD_FOOT, rs.ROD, order=32)      # (orders 32 and 64)
        print("sensor %d: closed form %.17g, quadrature %.17g" % (k, closed, quad))
        assert abs(closed - quad) <= 1e-16 and eps <= 1e-16
        assert abs(N * closed - rx.direct_reference("rod")["mu"][k]) <= 1e-9


def test_the_tolerances_of_the_rod():
    ref = rx.direct_reference("rod")
    rel = tolerance(ref) / ref["mu"]
    print("tolerance / mu:", rel)
    assert np.all(rel[:5] > 0.003) and np.all(rel[:5] < 0.0252) and rel[5] < 0.03


@pytest.mark.parametrize("name", tuple(rx.DIRECT_CASES))
def test_the_power_of_the_direct_cases(name):
    ref = rx.direct_reference(name)
    pw = rs.power(ref, tolerance(ref))
    print(name, pw)
    assert set(pw) >= {"no cosine", "2 pi for 4 pi", "rod at its midpoint", "a cosine on the spherical sensor", "two-sided planar"}
    assert min(pw.values()) >= 3.0, pw
    sphere = [k for k, (_, n) in enumerate(rx.ROD_SENSORS) if n is None]
    assert len(sphere) == 2 and np.all(ref["cosine_on_sphere"][sphere] == 0.0), "the spherical sensors in the rod's plane z = 0.7: a cosine gives exactly 0"


def test_the_power_of_the_plate_and_the_bounce():
    ref = rx.plate_reference()
    lit = ref["mu"] > 0
    tol = tolerance(ref)
    assert np.all(np.abs(ref["variants"]["2 pi for 4 pi"] - ref["mu"])[lit] >= 3.0 * tol[lit])
    assert np.all(ref["no_shadow_two_sided"][~lit] > 0), "no shadow, or a two-sided sensor: a reference of exactly 0 tells it apart"
    for call in rx.BOUNCE_CALLS:
        ref = rx.bounce_reference(call)
        pw = rs.power(ref, tolerance(ref))
        print(call, pw)
        assert min(pw.values()) >= 3.0, (call, pw)
    ref = rx.calibration_reference()
    assert min(rs.power(ref, tolerance(ref, K * rx.CALIBRATION_SAMPLES)).values()) >= 3.0


# ---------------------------------------------------------------- the restatement through the same cases
@pytest.mark.parametrize("mode", (0, 1))
@pytest.mark.parametrize("name", tuple(rx.DIRECT_CASES))
def test_the_restated_direct_gather(orc, name, mode):
    _, frm, to, length = rx.DIRECT_CASES[name]
    scene = ge.HandScene(orc, rx.direct_rows(name))
    sens = records(rx.ROD_SENSORS)
    got = np.array([gsr.gather(orc, scene, sens, frm, to, length, S, seed, N, mode=mode)[0] for seed in SEEDS])
    rs.accept("sensors, %s, mode %d" % (name, mode), got.mean(axis=0), rx.direct_reference(name), K * S)


def test_the_restated_plate(orc):
    scene = ge.HandScene(orc, rs.floor_rows(True))
    sens = records(rx.PLATE_SENSORS)
    ref = rx.plate_reference()
    got = np.array([gsr.gather(orc, scene, sens, rs.LAMP, rs.LAMP, 0.0, S, seed, N)[0] for seed in SEEDS])
    rs.accept("sensors, point lamp, plate", got.mean(axis=0), ref, K * S)
    dark = ref["mu"] == 0
    assert dark.sum() == 3 and np.all(got[:, dark] == 0.0) and not np.signbit(got[:, dark]).any()


@pytest.mark.parametrize("call", rx.BOUNCE_CALLS)
def test_the_restated_reflected_part(orc, call):
    scene = ge.HandScene(orc, rs.squares_rows())
    sens = records(rx.BOUNCE_SENSORS)
    source, faces, rho = rx.bounce_inputs(call)
    got = np.array([gsr.indirect(orc, scene, sens, S, seed, rs.BOUNCE_RHO, 0 if call == "source" else 1, source=source, faces=faces,
                                 rho_map=rho)[0] for seed in SEEDS])
    rs.accept("sensors, reflected, %s" % call, got.mean(axis=0), rx.bounce_reference(call), K * S)

// host_calls_sensors_check.cpp -- the host layer's call sequence with virtual dosimeters, without a GPU
// (tests/test_gather_sensors_cpu.py).  This is tests/tools/host_calls_check.cpp -- its stand-ins, its scene, its way of recording
// a case and a refusal, taken in whole by inclusion -- with recording stand-ins for the uvrt_* calls that
// host/raytracer_sensors.cpp makes and cases of its own: photons, gathers and every bounce model with sensors, driven
// segments, the sensors' own launch counter, uploads, a plan with sensors set, the calibration and every refusal.  It links
// host/raytracer_sensors.cpp beside the files host_calls_check links.  tests/golden/host_call_sequences_sensors.txt is its
// whole output; with a case's name that one alone.
#include <map>

#define main host_calls_check_main
#include "host_calls_check.cpp"
#undef main

namespace {
std::map<int, int> sensor_counts;                            // per context id: the sensors are the context's own, a scene swap leaves them
}

extern "C" {

// virtual dosimeters
int uvrt_sensor_info(uvrt_ctx* c, int32_t out4[4])
{
    out4[0] = sensor_counts.count(c->id) ? sensor_counts[c->id] : 0; out4[1] = out4[2] = out4[3] = 0;
    put("sensor_info c%d -> %d", c->id, out4[0]);
    return UVRT_OK;
}
int uvrt_set_sensors(uvrt_ctx* c, const uvrt_sensor* sensors, int32_t count)
{
    put("set_sensors c%d %s %d", c->id, A(sensors, (size_t)count * sizeof *sensors).c_str(), count);
    sensor_counts[c->id] = count;
    return UVRT_OK;
}
int uvrt_gather_sensors(uvrt_ctx* c, const uvrt_gather_params* g, int32_t first, int32_t count)
{
    put("gather_sensors c%d %s %d %d", c->id, G(*g).c_str(), first, count);
    return UVRT_OK;
}
int uvrt_gather_sensors_indirect(uvrt_ctx* c, const uvrt_sensor_indirect_params* p, int32_t first, int32_t count)
{
    put("gather_sensors_indirect c%d %08x %d %08x %d %d %d %d %d", c->id, F(p->reflectance), p->samples, p->seed, p->emitter,
        p->use_map, p->reserved, first, count);
    return UVRT_OK;
}
int uvrt_accumulate_sensors(uvrt_ctx* c, float dt) { put("accumulate_sensors c%d %08x", c->id, F(dt)); return UVRT_OK; }
int uvrt_reset_sensors(uvrt_ctx* c) { put("reset_sensors c%d", c->id); return UVRT_OK; }
int uvrt_read_sensor_plane(uvrt_ctx* c, int32_t which, double* out, int32_t first, int32_t count)
{
    put("read_sensor_plane c%d %d %d %d", c->id, which, first, count);
    for (int i = 0; i < count; ++i) out[i] = 4.0;
    return UVRT_OK;
}
int uvrt_sensor_dosage(uvrt_ctx* c, int32_t map, int32_t ppl, float power, float* out, int32_t first, int32_t count)
{
    put("sensor_dosage c%d %d %d %08x %d %d", c->id, map, ppl, F(power), first, count);
    for (int i = 0; i < count; ++i) out[i] = 0.5f;
    return UVRT_OK;
}
int uvrt_write_expected(uvrt_ctx* c, const double* in, int32_t first, int32_t count)
{
    put("write_expected c%d %s %d %d", c->id, A(in, (size_t)count * 8).c_str(), first, count);
    return UVRT_OK;
}
int uvrt_write_gather_faces(uvrt_ctx* c, int32_t face, const double* in, int32_t first, int32_t count)
{
    put("write_gather_faces c%d %d %s %d %d", c->id, face, A(in, (size_t)count * 8).c_str(), first, count);
    return UVRT_OK;
}

}  // extern "C"

namespace {

// three sensors: a planar one, a spherical one, a planar one looking down
void sensors(Scene& s)
{
    std::vector<uvrt_sensor> v(3);
    memset((void*)v.data(), 0, sizeof(uvrt_sensor) * v.size());
    v[0].pos[0] = 0.5f; v[0].pos[1] = 1.0f; v[0].pos[2] = -0.5f; v[0].normal[0] = -1.0f; v[0].kind = UVRT_SENSOR_PLANAR;
    v[1].pos[0] = -1.0f; v[1].pos[1] = 1.5f; v[1].pos[2] = 1.0f; v[1].kind = UVRT_SENSOR_SPHERICAL;
    v[2].pos[1] = 2.5f; v[2].normal[1] = -1.0f; v[2].kind = UVRT_SENSOR_PLANAR;
    s.rt.SetSensors(v);
    s.rt.sensorSamples = 8;
}
void read_sensors(Scene& s)
{
    std::vector<float> dose, peak;
    std::vector<double> err;
    s.rt.ReadSensors(dose, peak, err);
    put("-> sensors=%zu dose=%08x peak=%08x stdErr=%016llx", dose.size(), F(dose[0]), F(peak[0]), D(err[0]));
}

void list_sensor_cases()
{
    run("stops: photons + sensors", [](Scene& s) { sensors(s); s.reset_and_iterate(); read_sensors(s); });
    run("stops: gather + sensors", [](Scene& s) { sensors(s); gather(s, 4); s.rt.gatherSampling = 1; s.reset_and_iterate(); read_sensors(s); });
    run("stops: gather traced bounce + sensors", [](Scene& s) { sensors(s); gather(s, 4); bounce(s, 0.5f, 0, 0); s.rt.reflectSamples = 8; s.reset_and_iterate(); });
    run("stops: gather linked bounces + sensors", [](Scene& s) { sensors(s); gather(s, 4); bounce(s, 0.5f, 2, 0); s.reset_and_iterate(); });
    run("stops: gather sided bounces + sensors", [](Scene& s) { sensors(s); gather(s, 4); bounce(s, 0.5f, 2, 1); s.reset_and_iterate(); });
    run("stops: gather sided mapped bounces + sensors", [](Scene& s) { sensors(s); gather(s, 4); bounce(s, 0.5f, 2, 1); s.map(); s.reset_and_iterate(); });
    run("segments: photons + sensors", [](Scene& s) { sensors(s); s.rt.driveSpeed = 0.5f; s.rt.ResetDosageMap(); s.rt.ComputeSegments(); });
    run("segments: gather sided mapped bounces + sensors", [](Scene& s) {
        sensors(s); gather(s, 4); bounce(s, 0.5f, 2, 1); s.map(); s.rt.driveSpeed = 0.5f; s.rt.ResetDosageMap(); s.rt.ComputeSegments();
    });
    run("driving, two iterations: the sensors' own launch counter", [](Scene& s) {
        sensors(s); gather(s, 4); s.rt.driveSpeed = 0.5f; s.reset_and_iterate(); s.iterate(); s.rt.ResetDosageMap(); s.iterate();
    });
    run("gather batch 2 + sensors", [](Scene& s) { sensors(s); gather(s, 4); s.rt.gatherBatch = 2; s.reset_and_iterate(); });
    run("a scene swap keeps the sensors, a new context takes them again", [](Scene& s) {
        sensors(s); s.reset_and_iterate();
        uvrt_set_scene(s.rt.ctx, s.mesh.triangles, s.mesh.triangleCount, s.mesh.bvh->bvhNode, (int)s.mesh.bvh->nodesUsed, s.mesh.bvh->triIdx);
        s.iterate();
        s.rt.Init(&s.mesh); s.rt.ResetDosageMap(); s.iterate();
    });
    run("other sensors are uploaded, forgotten ones are gone", [](Scene& s) {
        sensors(s); s.reset_and_iterate(); sensors(s); s.iterate(); s.rt.SetSensors({}); s.iterate();
    });
    run("plan: counts with sensors set", [](Scene& s) { sensors(s); RayTracer::PlanOptions o; o.minDose = 50.0f; plan(s, o); });
    run("plan: gather with sensors set", [](Scene& s) { sensors(s); plan(s, gather_plan(4)); });
    run("calibrate at a sensor: photons", [](Scene& s) {
        sensors(s); s.rt.CalibratePowerAtSensor(3.0f, 1, 2); put("-> power=%08x intensity=%08x", F(s.rt.calibratedPower), F(s.rt.lightIntensity));
    });
    run("calibrate at a sensor: gather, traced bounce", [](Scene& s) { sensors(s); gather(s, 4); bounce(s, 0.5f, 0, 0); s.rt.CalibratePowerAtSensor(3.0f, 0, 0); });
    run("calibrate at a sensor: gather, sided mapped bounces", [](Scene& s) {
        sensors(s); gather(s, 4); bounce(s, 0.5f, 2, 1); s.map(); s.rt.sensorLaunches = 5; s.rt.CalibratePowerAtSensor(3.0f, 2, 1);
        put("-> sensorLaunches=%u", s.rt.sensorLaunches);
    });

    refuse("sensors: launch sharding", [](Scene& s) { sensors(s); s.rt.shardWorld = 2; s.reset_and_iterate(); });
    refuse("sensors: ComputeIterationsBatched", [](Scene& s) { sensors(s); s.rt.ResetDosageMap(); s.rt.ComputeIterationsBatched(1); });
    refuse("sensors: a group", [](Scene& s) { Scene other; sensors(other); RayTracer::ComputeIterationsBatched({&s.rt, &other.rt}, 1); });
    refuse("sensors: reduceOverComm", [](Scene& s) { sensors(s); s.rt.reduceOverComm = true; s.reset_and_iterate(); });
    refuse("sensors: mirror panels", [](Scene& s) { sensors(s); gather(s, 4); s.mirrors(); s.reset_and_iterate(); });
    refuse("sensors: a rules file that is not there", [](Scene& s) { s.rt.sensorMap = "no_such_file"; s.reset_and_iterate(); });
    refuse("sensors: ReadSensors without sensors", [](Scene& s) { std::vector<float> a, b; std::vector<double> c; s.rt.ReadSensors(a, b, c); });
    refuse("calibrate at a sensor: no sensors", [](Scene& s) { s.rt.CalibratePowerAtSensor(3.0f, 0, 0); });
    refuse("calibrate at a sensor: no such sensor", [](Scene& s) { sensors(s); s.rt.CalibratePowerAtSensor(3.0f, 3, 0); });
    refuse("calibrate at a sensor: no such lamp", [](Scene& s) { sensors(s); s.rt.CalibratePowerAtSensor(3.0f, 0, 3); });
    refuse("calibrate at a sensor: mirror panels", [](Scene& s) { sensors(s); gather(s, 4); s.mirrors(); s.rt.CalibratePowerAtSensor(3.0f, 0, 0); });
    refuse("calibrate at a sensor: reflectance with photons", [](Scene& s) { sensors(s); bounce(s, 0.5f, 0, 0); s.rt.CalibratePowerAtSensor(3.0f, 0, 0); });
}

}  // namespace

int main(int argc, char** argv)
{
    omp_set_num_threads(1);
    out = fdopen(dup(1), "w");
    if (!out || !freopen("/dev/null", "w", stdout)) return 3;
    (void)host_calls_check_main;
    list_sensor_cases();
    cases.insert(cases.begin(), {"set-up", [](Scene&) {}, false});
    bool found = false;
    for (const Case& c : cases) {
        if (argc > 1 && c.name != argv[1]) continue;
        found = true;
        sensor_counts.clear();
        std::string text;
        if (c.name == "set-up") {
            contexts = 0;
            record.clear();
            { Scene s; }
            text = record;
        } else {
            text = c.refusal ? refused(c) : recorded(c);
        }
        fprintf(out, "== %s\n%s", c.name.c_str(), text.c_str());
    }
    if (!found) { fprintf(stderr, "no case '%s'\n", argv[1]); return 2; }
    return fclose(out) == 0 ? 0 : 3;
}

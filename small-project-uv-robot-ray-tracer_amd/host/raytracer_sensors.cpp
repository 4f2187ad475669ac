// raytracer_sensors.cpp -- the virtual dosimeters of the host layer (raytracer.h sensorMap): the rules file, the
// upload, the sensors' part of a launch, ReadSensors and CalibratePowerAtSensor.  Every uvrt_* sensor call of the host layer
// is made here.  raytracer.cpp reaches this file through RayTracer::sensorHooks alone, which InstallSensorHooks below sets
// when the file is part of the program (libuvrt_host.so always holds it): a program built without it runs every path that
// has no sensors as before and refuses sensors.
#include "raytracer.h"
#include "raytracer_internal.h"

#include "../../include/uvrt.h"

#include <algorithm>
#include <cmath>
#include <cstring>
#include <fstream>
#include <sstream>

using namespace Tmpl8;
using namespace Tmpl8::host_internal;

bool RayTracer::InstallSensorHooks()
{
    static const SensorHooks hooks = {&RayTracer::GatherSensors, &RayTracer::ResetSensors};
    sensorHooks = &hooks;
    return true;
}
static const bool sensor_hooks_installed = RayTracer::InstallSensorHooks();

void RayTracer::ResetSensors()
{
    UploadSensors();
    check(uvrt_reset_sensors(ctx), "reset_sensors");
    sensorLaunches = 0;
}

std::string RayTracer::ParseSensorRules(const char* path, std::vector<uvrt_sensor>* out)
{
    std::ifstream f(path, std::ios::binary);
    if (!f) return std::string(path) + ": cannot be read";
    out->clear();
    std::string line;
    for (int no = 1; std::getline(f, line); ++no) {
        auto bad = [&](const std::string& why) { return std::string(path) + ":" + std::to_string(no) + ": " + why; };
        std::istringstream ss(line.substr(0, line.find('#')));
        std::vector<std::string> w;
        for (std::string word; ss >> word;) w.push_back(word);
        if (w.empty()) continue;
        const bool grid = w[0] == "grid";
        if (!grid && w[0] != "sensor") return bad("unknown keyword '" + w[0] + "'");
        const size_t at = grid ? 10 : 4;                     // where the kind stands
        const char* form = grid ? "grid takes X0 Y0 Z0 X1 Y1 Z1 NX NY NZ sphere | planar MX MY MZ" : "sensor takes X Y Z sphere | planar NX NY NZ";
        if (w.size() <= at) return bad(form);
        const bool planar = w[at] == "planar";
        if (!planar && w[at] != "sphere") return bad("unknown kind '" + w[at] + "' (planar or sphere)");
        if (w.size() != at + (planar ? 4 : 1)) return bad(form);
        float v[6], n[3] = {0.0f, 0.0f, 0.0f};
        for (size_t k = 0; k < (grid ? 6u : 3u); ++k)
            if (!rule_number(w[1 + k], &v[k]) || !std::isfinite(v[k])) return bad("'" + w[1 + k] + "' is not a finite number");
        for (size_t k = 0; planar && k < 3; ++k)
            if (!rule_number(w[at + 1 + k], &n[k]) || !std::isfinite(n[k])) return bad("'" + w[at + 1 + k] + "' is not a finite number");
        if (planar && n[0] == 0.0f && n[1] == 0.0f && n[2] == 0.0f) return bad("a planar sensor's normal is zero");
        long long cells[3] = {1, 1, 1};
        for (size_t k = 0; grid && k < 3; ++k) {
            char* end = nullptr;
            cells[k] = strtoll(w[7 + k].c_str(), &end, 10);
            if (end != w[7 + k].c_str() + w[7 + k].size() || cells[k] < 1 || cells[k] > UVRT_SENSOR_MAX)
                return bad("'" + w[7 + k] + "' is not an integer >= 1");
        }
        if ((long long)out->size() + cells[0] * cells[1] * cells[2] > UVRT_SENSOR_MAX)
            return bad("more than " + std::to_string(UVRT_SENSOR_MAX) + " sensors");
        uvrt_sensor rec;
        memset(&rec, 0, sizeof rec);
        rec.kind = planar ? UVRT_SENSOR_PLANAR : UVRT_SENSOR_SPHERICAL;
        for (int k = 0; k < 3; ++k) rec.normal[k] = n[k];
        if (!grid) {
            for (int k = 0; k < 3; ++k) rec.pos[k] = v[k];
            out->push_back(rec);
            continue;
        }
        for (long long iz = 0; iz < cells[2]; ++iz)
            for (long long iy = 0; iy < cells[1]; ++iy)
                for (long long ix = 0; ix < cells[0]; ++ix) {
                    rec.pos[0] = v[0] + (v[3] - v[0]) * (((float)ix + 0.5f) / (float)cells[0]);
                    rec.pos[1] = v[1] + (v[4] - v[1]) * (((float)iy + 0.5f) / (float)cells[1]);
                    rec.pos[2] = v[2] + (v[5] - v[2]) * (((float)iz + 0.5f) / (float)cells[2]);
                    out->push_back(rec);
                }
    }
    return std::string();
}

void RayTracer::SetSensors(const std::vector<uvrt_sensor>& sensors)
{
    if (sensors.size() > (size_t)UVRT_SENSOR_MAX) fatal("SetSensors: at most 2^24 sensors");
    sensorList = sensors;
    sensorValuesStamp = sensorStampNext++;
}

std::string RayTracer::SensorMapPath() const
{
    return sensorMap.empty() || sensorMap[0] == '/' ? sensorMap : routeDir + sensorMap;
}

std::string RayTracer::PrepareSensorMap()
{
    if (sensorMap.empty()) return std::string();
    const std::string path = SensorMapPath();
    if (sensorFileParsed == path) return std::string();
    sensorFileParsed.clear();
    const std::string err = ParseSensorRules(path.c_str(), &sensorFileList);
    if (!err.empty()) { sensorFileList.clear(); return err; }
    if (sensorFileList.empty()) return path + ": no sensor";
    sensorFileParsed = path;
    sensorFileStamp = sensorStampNext++;
    return std::string();
}

const std::vector<uvrt_sensor>& RayTracer::ActiveSensors() const
{
    static const std::vector<uvrt_sensor> none;
    if (sensorMap.empty()) return sensorList;
    return sensorFileParsed == SensorMapPath() ? sensorFileList : none;
}

void RayTracer::UploadSensors()
{
    const std::string err = PrepareSensorMap();
    if (!err.empty()) fatal(("sensorMap: " + err).c_str());
    const std::vector<uvrt_sensor>& sensors = ActiveSensors();
    const unsigned long long stamp = sensorMap.empty() ? sensorValuesStamp : sensorFileStamp;
    if (sensors.empty()) fatal("the sensor gather needs sensors (sensorMap or SetSensors)");
    int32_t info[4];
    check(uvrt_sensor_info(ctx, info), "sensor_info");
    if (info[0] > 0 && sensorUploaded == stamp) return;
    check(uvrt_set_sensors(ctx, sensors.data(), (int32_t)sensors.size()), "set_sensors");
    sensorUploaded = stamp;
}

void RayTracer::GatherSensors(const RouteLaunch& l, int photons, const GatherOptions& opt, unsigned gatherSeed, bool accumulate)
{
    CheckSensorsAlone("sensors");
    UploadSensors();
    const int32_t K = (int32_t)ActiveSensors().size();
    const uvrt_gather_params g = gather_params(l, lightLength, sensorSamples, sensorLaunches++, photons);
    check(uvrt_set_gather_sampling(ctx, gatherSampling), "set_gather_sampling");
    check(uvrt_gather_sensors(ctx, &g, 0, K), "gather_sensors");
    if (opt.samples > 0 && opt.reflectance > 0.0f) {
        // one diffuse bounce in both bounce models: the two-sided ones have left the direct plane's snapshot in the source
        // plane, the face-resolved ones the direct gather's face planes
        uvrt_sensor_indirect_params ip;
        memset(&ip, 0, sizeof ip);
        ip.reflectance = opt.reflectance;
        ip.samples = opt.reflectSamples;
        ip.seed = gatherSeed ^ 0x85EBCA6Bu;
        ip.emitter = opt.sided != 0 ? 1 : 0;
        ip.use_map = opt.sided != 0 && opt.mapped ? 1 : 0;
        check(uvrt_gather_sensors_indirect(ctx, &ip, 0, K), "gather_sensors_indirect");
    }
    if (accumulate) check(uvrt_accumulate_sensors(ctx, l.duration), "accumulate_sensors");
}

void RayTracer::ReadSensors(std::vector<float>& dose, std::vector<float>& peak, std::vector<double>& stdErr)
{
    if (!HasSensors()) fatal("ReadSensors: no sensors (sensorMap or SetSensors)");
    UploadSensors();
    const int32_t K = (int32_t)ActiveSensors().size();
    const ViewMode keep = viewMode;
    viewMode = dosage;
    const ShadeArguments d = ShadeArgs();
    viewMode = maxpower;
    const ShadeArguments m = ShadeArgs();
    viewMode = keep;
    dose.assign((size_t)K, 0.0f);
    peak.assign((size_t)K, 0.0f);
    std::vector<double> var((size_t)K, 0.0);
    check(uvrt_sensor_dosage(ctx, d.which_map, d.photons_per_light, d.scaled_power, dose.data(), 0, K), "sensor_dosage");
    check(uvrt_sensor_dosage(ctx, m.which_map, m.photons_per_light, m.scaled_power, peak.data(), 0, K), "sensor_dosage");
    check(uvrt_read_sensor_plane(ctx, 4, var.data(), 0, K), "read_sensor_plane");
    stdErr.assign((size_t)K, 0.0);
    for (int32_t k = 0; k < K; ++k) stdErr[(size_t)k] = (double)d.scaled_power * sqrt(var[(size_t)k]) / (double)d.photons_per_light;
}

void RayTracer::CalibratePowerAtSensor(float measurePower, int sensor, int lightIndex)
{
    if (!HasSensors()) fatal("CalibratePowerAtSensor: no sensors (sensorMap or SetSensors)");
    if (lightIndex < 0 || (size_t)lightIndex >= lightPositions.size()) fatal("CalibratePowerAtSensor: no such lamp position");
    CheckSensorsAlone("CalibratePowerAtSensor");
    UploadSensors();
    if (sensor < 0 || (size_t)sensor >= ActiveSensors().size()) fatal("CalibratePowerAtSensor: no such sensor");
    const GatherOptions opt = OwnGather();
    if (const char* why = GatherRefusal(opt, kLaunchRefusals, false)) fatal(why);
    const int T = mesh->triangleCount;
    const RouteLaunch l = RouteLaunches({lightPositions[(size_t)lightIndex]}, mesh->floorHeight + lightHeight, 0.0f)[0];
    check(uvrt_reset_sensors(ctx), "reset_sensors");
    const unsigned keepLaunches = sensorLaunches;
    sensorLaunches = 0;
    const bool bounce = opt.samples > 0 && opt.reflectance > 0.0f;
    if (bounce) {
        // what the sensors' bounce reads: the launch's direct plane as the source plane, or its face planes.  The planes this
        // leaves behind are zeroed again below: between launches they are zero.
        const uvrt_gather_params g = gather_params(l, lightLength, opt.samples, 0u, photonCount);
        check(uvrt_set_gather_sampling(ctx, opt.sampling), "set_gather_sampling");
        int32_t faces = 0;                                   // (reflectSided: the faces state on around it, then put back)
        if (opt.sided != 0) {
            check(uvrt_get_gather_faces(ctx, &faces), "get_gather_faces");
            check(uvrt_set_gather_faces(ctx, 1), "set_gather_faces");
        }
        check(uvrt_gather_direct(ctx, &g, 0, T), "gather_direct");
        if (opt.sided != 0) check(uvrt_set_gather_faces(ctx, faces), "set_gather_faces");
        if (opt.sided == 0) check(uvrt_indirect_source_from_expected(ctx), "indirect_source_from_expected");
        else if (opt.mapped) UploadReflectanceMap(T, opt.reflectance);
    }
    GatherSensors(l, photonCount, opt, 0u, false);
    check(uvrt_accumulate_sensors(ctx, 1.0f), "accumulate_sensors");
    if (bounce) {
        const std::vector<double> zero((size_t)T, 0.0);
        check(uvrt_write_expected(ctx, zero.data(), 0, T), "write_expected");
        if (opt.sided != 0)
            for (int f = 0; f < 2; ++f) check(uvrt_write_gather_faces(ctx, f, zero.data(), 0, T), "write_gather_faces");
    }
    float value = 0.0f;                                      // power 1, so measured / gathered irradiance is the calibrated power
    check(uvrt_sensor_dosage(ctx, UVRT_MAP_MAX, photonCount, 1.0f, &value, sensor, 1), "sensor_dosage");
    check(uvrt_reset_sensors(ctx), "reset_sensors");
    sensorLaunches = keepLaunches;
    if (!(value > 0.0f)) fatal("CalibratePowerAtSensor: the sensor receives nothing from that lamp position");
    calibratedPower = 0.01f * (measurePower / value);
    lightIntensity = calibratedPower;
}

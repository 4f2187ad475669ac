// uvrt_cli.cpp -- headless equivalent of the reference's per-frame compute block
// (MyApp::Init myapp.cpp:36-39 + MyApp::Tick myapp.cpp:156-175): load the room, Init the
// RayTracer, ResetDosageMap, then {ComputeDosageMap; Shade; currIterations++; sync; progress
// line} until maxIterations, and dump the per-triangle dose.
//
//   uvrt_cli --room rooms/testroomopt.glb [--route-dir positions/] [--route lange_route]
//            [--photons N] [--iterations K] [--lamps L] [--view dosage|maxpower]
//            [--calibrate POWER HEIGHT DIST] [--device D] [--save-route name]
//            [--dump dose.f32 | dose.npy]   raw little-endian f32[T] or NumPy .npy (by extension)
//            [--ply heatmap.ply]            the room with per-triangle heat-map colours
//                                           (dosageToColor output; what the reference shows in GL)
//            [--flavour 0|1|2]              arithmetic of extend (include/uvrt.h uvrt_set_flavour): 0 strict (default), 1 the fused
//                                           forms of the reference's strict build on gfx950, 2 what the reference's OWN build
//                                           flags (-cl-fast-relaxed-math, template.cpp:1192) compute on gfx950 (+11 %)
//            [--batch K]                    trace K iterations per batch (RayTracer::ComputeIterationsBatched:
//                                           all launches first, accumulate + Shade replayed; same dose bits)
//            [--gpus N]                     one process, N contexts: every launch split by global-id range
//                                           ("pixel tiles"), ONE RCCL all-reduce of the count planes per batch
//                                           (contexts share a device when the box has fewer than N: no RCCL then)
//            [--plan [MIN_DOSE]]            plan the durations (RayTracer::PlanDurations): least total time that brings every
//                                           required triangle to MIN_DOSE mJ/cm^2 (default: the route's minimale_dosis);
//                                           prints the report, --save-route saves the planned route, --dump the plan's model dose
//            [--candidates grid:NX,NZ[,INSET]]  plan over an NX x NZ grid over the room's x/z bounds (inset, metres: 0.5)
//            [--min-photons N]              triangles with fewer captured photons are "unresolved", not required (16)
//            [--plan-verify]                recompute from the plan's SEED with the planned durations through the normal
//                                           pipeline and count the required triangles below the minimum (exit 1 unless 0)
//            [--verify-dump FILE]           the dose of that recompute (raw f32 or .npy)
//            [--plan-holdout SEED]          the same from another SEED: area fraction at or above the minimum (informative)
//            [--drive-speed V]              the lamp radiates while the robot drives between consecutive positions at V m/s
//                                           (RayTracer::driveSpeed; default: the route's <rijsnelheid>, 0 = stops only);
//                                           one context; with --plan use --plan-drive
//            [--plan-drive V]               plan (as --plan) for a route driven at V m/s: the segments between consecutive
//                                           positions are fixed columns of the plan at the time the drive takes, so the stops
//                                           only add what the drive leaves missing; sets the route's speed (--save-route
//                                           writes <rijsnelheid>); 0 forces a stops-only plan of a route file that drives.
//                                           A route file whose own <rijsnelheid> is > 0 is planned with driving under --plan.
//                                           At most 128 positions, one context.
//            [--gather S]                   the direct gather in place of photon counting (RayTracer::gatherSamples; default:
//                                           the route's <gather_samples>, 0 = photons): every stop and every driven segment
//                                           is S shadow rays per triangle towards the lamp, so the dim triangles that no photon
//                                           reaches get an estimate too; one context, launch by launch: refused with --batch,
//                                           --gpus > 1, --plan and --plan-drive
//            [--plan-gather S]              plan (as --plan; with --plan MIN for that minimum, with --plan-drive V for a driven
//                                           route) with the exposure from the direct gather, S in [1, 4096] shadow rays per
//                                           triangle and launch (RayTracer::PlanOptions::gatherSamples): the triangles no photon
//                                           reaches are planned for too.  --candidates, --min-photons, --dump and --verify-dump
//                                           work as with --plan; --plan-verify recomputes with gatherSamples = S; --save-route
//                                           saves the planned route with <gather_samples>S.  The plan is as good as the
//                                           estimator: raise S or the margin for a tighter one.  One context,
//                                           launch by launch: refused with --gather, --batch, --gpus > 1 and --plan-holdout
//            [--gather-sampling independent|stratified]
//                                           how the gather places its S samples on the lamp (RayTracer::gatherSampling,
//                                           PlanOptions::gatherSampling; default: the route's <gather_sampling>, independent):
//                                           stratified puts sample s into stratum s of the rod and the sweep coordinate on a
//                                           rotated golden-ratio sequence -- the same shadow rays, at a stop an estimate about as
//                                           tight as four times the samples.  Needs --gather S or --plan-gather S
//            [--plan-confidence Z]          with --plan-gather S, S >= 2: plan for the lower confidence bound of the gather's
//                                           estimate, expected - Z standard errors element by element (PlanOptions::
//                                           gatherConfidence): every required triangle reaches the minimum with
//                                           that confidence in the estimator, not just for the estimate.  Z finite and >= 0
//                                           (0: the plan without it); meant for S >= 16 -- at S = 4 about half the bounds are 0.
//                                           --plan-verify recomputes with the plain gather of the same seeds, whose estimate is
//                                           >= the bound element by element, so the plan holds there
//            [--gather-refine TAU[,MAX]]    with --gather S or --plan-gather S, S >= 2: the adaptive gather (RayTracer::
//                                           gatherRelError / gatherMaxExtra, PlanOptions::gatherRelError / gatherMaxExtra, DESIGN.md
//                                           16): after every gather launch the triangles whose standard error exceeds TAU times
//                                           their estimate get up to MAX extra shadow rays (a power of two in [2, 4096], default
//                                           64).  TAU finite and > 0.  With --plan-gather, --plan-verify recomputes with the same
//                                           refine, so it sees the plan's own estimates; works with and without --plan-confidence
//            [--reflect RHO[,S2]]           with --gather S or --plan-gather S (also under --drive-speed / --plan-drive): one diffuse
//                                           bounce on top of every gather launch (RayTracer::reflectance / reflectSamples,
//                                           PlanOptions::reflectance / reflectSamples): S2 cosine-distributed rays per
//                                           triangle (even, in [2, 4096], default 16) look up what their closest hit receives
//                                           directly; RHO in [0, 1] is the one reflectance of every surface.  The triangles behind
//                                           furniture that see no lamp get an estimate.  One bounce; the variance plane stays the
//                                           direct part's, so --plan-confidence refuses it.  --save-route writes <reflectance> and
//                                           <reflect_samples>; --plan-verify recomputes with the same bounce
//            [--reflect-bounces K]          with --reflect: K bounces in [1, 16] over hit links recorded once per scene instead of
//                                           the one bounce traced per launch (RayTracer::reflectBounces, PlanOptions::reflectBounces,
//                                           DESIGN.md 18): the bounce's rays are traced once with S2 samples and a fixed seed, every
//                                           launch then looks its sources up along them, and bounces 2..K come with it.  All launches
//                                           see the same directions: the bounce's sampling error no longer averages out over a
//                                           route, but S2 is paid once and can be much larger.  --save-route writes <reflect_bounces>
//            [--reflect-sided]              with --reflect RHO > 0 and --reflect-bounces K: the K bounces are face-resolved
//                                           (RayTracer::reflectSided, PlanOptions::reflectSided): every triangle is an
//                                           opaque sheet whose two faces keep their own irradiance, so the bounces conserve energy
//                                           at every RHO.  Refused without --reflect-bounces (the traced single bounce has no such
//                                           form), with RHO = 0 and with --gather-batch B >= 2.  --save-route writes <reflect_sided>
//            [--reflect-map FILE]           with --reflect-sided: a reflectance per face in place of the one RHO (RayTracer::reflectMap,
//                                           PlanOptions::reflectMapped).  FILE holds lines "box X0 Y0 Z0 X1 Y1 Z1 RHO"
//                                           (both faces of every triangle whose centroid lies in the closed box) and "box .. RHO
//                                           toward PX PY PZ" (only the face that looks at P); later lines override earlier ones, #
//                                           starts a comment, every face starts at --reflect's RHO.  A relative FILE is resolved
//                                           against --route-dir.  Refused without --reflect-sided.  --save-route writes <reflect_map>
//            [--sensors FILE]               virtual dosimeters (RayTracer::sensorMap): lines "sensor X Y Z planar NX NY NZ",
//                                           "sensor X Y Z sphere" and "grid X0 Y0 Z0 X1 Y1 Z1 NX NY NZ sphere | planar MX MY MZ"; every
//                                           launch, photons or gather, also gathers the lamp's light and one diffuse bounce at them.
//                                           Refused with --mirror-map, --gpus > 1 and --batch.  --save-route writes <sensor_map>
//            [--sensor-samples S]           shadow rays per sensor and launch (default 64)
//            [--sensor-dump OUT.csv]        index, kind, position, normal, dose (mJ/cm^2), peak (uW/cm^2), standard error of dose
//            [--calibrate-sensor P K I]     lamp power from a reading P at sensor K with the lamp at position I, in the room as it is
//            [--mirror-map FILE]            with --gather S or --plan-gather S: specular reflector panels (RayTracer::mirrorMap,
//                                           PlanOptions::mirrorMapped).  FILE holds lines "mirror X0 Y0 Z0 X1 Y1 Z1 RHO
//                                           plane QX QY QZ MX MY MZ": the next panel (8 at most) is the plane through Q with normal
//                                           M, it reflects on the side M points to with the specular reflectance RHO, and the
//                                           triangles whose centroid lies in the closed box are where it is a mirror; # starts a
//                                           comment.  After every gather launch the lamp's mirror image in every panel is gathered
//                                           into the launch's plane (two traced legs per sample), before the diffuse bounces.  A
//                                           relative FILE is resolved against --route-dir.  Refused with --plan-confidence (the
//                                           variance plane is the direct part's).  --save-route writes <mirror_map>
//            [--gather-batch B]             with --gather S or --plan-gather S: trace the gather launches in groups of up to B in
//                                           [0, 64] (RayTracer::gatherBatch, PlanOptions::gatherBatch): one shadow-ray
//                                           pass per group instead of one per launch.  0 (default) and 1: launch by launch.  B
//                                           changes no bit of the dose, the plan or its report, and is not saved in route files
#include "raytracer.h"
#include "../../include/uvrt.h"

#include <algorithm>
#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <fstream>
#include <iostream>
#include <vector>

using namespace Tmpl8;

namespace {

void write_f32(const std::string& path, const std::vector<float>& v)
{
    std::ofstream f(path, std::ios::binary);
    if (path.size() > 4 && path.substr(path.size() - 4) == ".npy") {
        // NumPy format 1.0: magic, version, header length, dict padded to a 64-byte boundary
        std::string hdr = "{'descr': '<f4', 'fortran_order': False, 'shape': (" + std::to_string(v.size()) + ",), }";
        while ((10 + hdr.size() + 1) % 64) hdr += ' ';
        hdr += '\n';
        const unsigned short hl = (unsigned short)hdr.size();
        f.write("\x93NUMPY\x01\x00", 8);
        f.write((const char*)&hl, 2);
        f.write(hdr.data(), (std::streamsize)hdr.size());
    }
    f.write((const char*)v.data(), (std::streamsize)v.size() * 4);
}

// --save-route: the first 31 characters of the name, as SaveRoute takes it
void save_route(RayTracer& rt, const std::string& name)
{
    if (name.empty()) return;
    char buf[32];
    strncpy(buf, name.c_str(), 31);
    buf[31] = 0;
    rt.SaveRoute(buf);
}

// the route's computation from `seed` with the current durations (batched or per launch), dose read back
std::vector<float> recompute(RayTracer& rt, uint32_t seed, int batch)
{
    if (uvrt_set_seed(rt.ctx, seed) != UVRT_OK) { fprintf(stderr, "set_seed: %s\n", uvrt_last_error()); exit(1); }
    rt.ResetDosageMap();
    rt.viewMode = dosage;
    while (rt.currIterations < rt.maxIterations) {
        if (batch > 0) {
            RayTracer::ComputeIterationsBatched(std::vector<RayTracer*>{&rt}, std::min(batch, rt.maxIterations - rt.currIterations));
        } else {
            rt.ComputeDosageMap();
            rt.Shade();
            rt.currIterations++;
        }
    }
    std::vector<float> dose(rt.mesh->triangleCount);
    rt.ReadDosage(dose.data(), 0, rt.mesh->triangleCount);
    return dose;
}

int run_plan(RayTracer& rt, float minDose, int minPhotons, bool verify, bool holdout, uint32_t holdoutSeed, int batch,
             const std::string& dump, const std::string& verifyDump, int planGather, int gatherSampling, double planConfidence,
             double refineTau, int refineMax, float reflect, int reflectS, int reflectK, int reflectSided, int reflectMapped,
             int mirrorMapped)
{
    const int T = rt.mesh->triangleCount;
    RayTracer::PlanOptions opt;
    opt.minDose = minDose;
    opt.minPhotons = minPhotons;
    opt.gatherSamples = planGather;
    opt.gatherSampling = planGather > 0 ? gatherSampling : 0;
    opt.gatherConfidence = planGather > 0 ? planConfidence : 0.0;
    opt.gatherRelError = planGather > 0 ? refineTau : 0.0;
    opt.gatherMaxExtra = refineMax;
    opt.reflectance = planGather > 0 ? reflect : 0.0f;
    opt.reflectSamples = reflectS;
    opt.reflectBounces = planGather > 0 ? reflectK : 0;
    opt.reflectSided = planGather > 0 ? reflectSided : 0;
    opt.reflectMapped = planGather > 0 ? reflectMapped : 0;
    opt.mirrorMapped = planGather > 0 ? mirrorMapped : 0;
    opt.gatherBatch = planGather > 0 ? rt.gatherBatch : 0;   // (--gather-batch: --plan-verify recomputes in the same groups)
    unsigned seed0 = 0;
    const uvrt_plan_report r = rt.PlanDurations(opt, &seed0);
    if (planGather > 0) {
        rt.gatherSamples = planGather;       // the planned route is a gather route: --plan-verify and --save-route
        rt.gatherSampling = opt.gatherSampling;
        printf("plan: exposure from the direct gather, %d samples per triangle and launch\n", planGather);
        if (opt.gatherSampling == UVRT_GATHER_STRATIFIED) printf("plan: stratified gather sampling\n");
        if (opt.gatherConfidence > 0.0) printf("plan: lower confidence bound, z = %.9g\n", opt.gatherConfidence);
        if (opt.mirrorMapped) printf("plan: specular panels %s\n", rt.mirrorMap.c_str());
        if (opt.gatherRelError > 0.0) {
            rt.gatherRelError = opt.gatherRelError;     // --plan-verify recomputes the plan's own estimates
            rt.gatherMaxExtra = opt.gatherMaxExtra;
            printf("plan: adaptive gather, relative error %.9g, at most %d extra samples\n", opt.gatherRelError, opt.gatherMaxExtra);
        }
        if (opt.reflectance > 0.0f) {
            rt.reflectance = opt.reflectance;           // --plan-verify and --save-route: the plan's own bounce
            rt.reflectSamples = opt.reflectSamples;
            rt.reflectBounces = opt.reflectBounces;
            rt.reflectSided = opt.reflectSided;
            if (opt.reflectSided) printf("plan: face-resolved bounces\n");
            if (opt.reflectMapped) printf("plan: reflectance map %s over the base reflectance\n", rt.reflectMap.c_str());
            if (opt.reflectBounces > 0)
                printf("plan: %d diffuse bounces over recorded hit links, reflectance %.8g, %d samples per triangle\n", opt.reflectBounces, (double)opt.reflectance, opt.reflectSamples);
            else
                printf("plan: one diffuse bounce, reflectance %.8g, %d samples per triangle and launch\n", (double)opt.reflectance, opt.reflectSamples);
        }
    }
    const float m = minDose >= 0.0f ? minDose : rt.minDosage;
    printf("plan: %d positions, %d used, total duration %.9g (lower bound %.9g, gap %.3g), %s after %d iterations\n",
           r.positions, r.used_positions, r.total_duration, r.lower_bound, r.gap,
           r.status == UVRT_PLAN_CONVERGED ? "converged" : "iteration cap", r.iterations);
    if (rt.planBounds.fixed_columns > 0)
        printf("plan: driving at %.9g m/s: drive time %.9g s over %d segments; %d rows met by the drive alone (area %.6g), "
               "%d short rows no stop reaches (area %.6g)\n", (double)rt.driveSpeed, rt.planBounds.lower_total,
               rt.planBounds.fixed_columns, rt.planBounds.met_by_lower, rt.planBounds.area_met_by_lower,
               rt.planBounds.short_rows, rt.planBounds.area_short);
    printf("plan: minimum %.9g mJ/cm^2 from SEED %u; required %d triangles (area %.6g), unreachable %d (area %.6g), "
           "unresolved %d (area %.6g), masked out %d (area %.6g); min dose / minimum %.9g\n",
           (double)m, seed0, r.required, r.area_required, r.unreachable, r.area_unreachable, r.unresolved, r.area_unresolved,
           r.masked_out, r.area_masked_out, r.min_dose_ratio);
    for (size_t i = 0; i < rt.lightPositions.size(); ++i)
        if (rt.lightPositions[i].duration > 0.0f)
            printf("plan: position %zu (%.6g, %.6g) duration %.9g\n", i, rt.lightPositions[i].position.x,
                   rt.lightPositions[i].position.y, rt.lightPositions[i].duration);
    std::vector<float> d(rt.lightPositions.size());           // every column of the plan: the stops, then the segments
    for (size_t i = 0; i < d.size(); ++i) d[i] = rt.lightPositions[i].duration;
    if (rt.planBounds.fixed_columns > 0) d.insert(d.end(), rt.planSegmentDurations.begin(), rt.planSegmentDurations.end());
    std::vector<uint8_t> req(T);
    if (uvrt_plan_read_required(rt.ctx, req.data(), 0, T) != UVRT_OK) { fprintf(stderr, "plan: %s\n", uvrt_last_error()); return 1; }
    if (!dump.empty()) {
        std::vector<float> model(T);
        if (uvrt_plan_model_dose(rt.ctx, d.data(), model.data(), 0, T) != UVRT_OK) { fprintf(stderr, "plan: %s\n", uvrt_last_error()); return 1; }
        write_f32(dump, model);
    }
    int rc = 0;
    if (verify) {
        const std::vector<float> dose = recompute(rt, seed0, batch);
        int below = 0;
        for (int t = 0; t < T; ++t) below += req[t] && !(dose[t] >= m);
        printf("plan-verify: %d below minimum of %d required triangles (SEED %u)\n", below, r.required, seed0);
        if (!verifyDump.empty()) write_f32(verifyDump, dose);
        if (below) rc = 1;
    }
    if (holdout) {
        const std::vector<float> dose = recompute(rt, holdoutSeed, batch);
        double a_req = 0, a_ok = 0;
        for (int t = 0; t < T; ++t) {
            if (!req[t]) continue;
            // the context's f32 area (k_prepare_scene: same operations, same order; this file builds with -ffp-contract=off)
            const Tri& tr = rt.mesh->triangles[t];
            const float ax = tr.vertex0.x - tr.vertex1.x, ay = tr.vertex0.y - tr.vertex1.y, az = tr.vertex0.z - tr.vertex1.z;
            const float bx = tr.vertex0.x - tr.vertex2.x, by = tr.vertex0.y - tr.vertex2.y, bz = tr.vertex0.z - tr.vertex2.z;
            const float cx = ay * bz - az * by, cy = az * bx - ax * bz, cz = ax * by - ay * bx;
            const double a = std::sqrt(cx * cx + cy * cy + cz * cz) / 2.0f;
            a_req += a;
            if (dose[t] >= m) a_ok += a;
        }
        printf("plan-holdout: SEED %u, area fraction at or above minimum %.6f\n", holdoutSeed, a_req > 0 ? a_ok / a_req : 1.0);
    }
    return rc;
}

}  // namespace

int main(int argc, char** argv)
{
    std::string room, routeDir = "positions/", route = "route", dump, saveRoute, ply;
    long long photons = -1;
    int iterations = -1, lamps = -1, device = 0, gpus = 1, batch = 0, flavour = 0;
    bool calibrate = false, plan = false, planVerify = false, planHoldout = false;
    float planMin = -1.0f, gridInset = 0.5f, driveSpeed = -1.0f, planDrive = -1.0f;
    int minPhotons = 16, gridX = 0, gridZ = 0, gather = -1, planGather = 0, gatherSampling = -1;
    uint32_t holdoutSeed = 0;
    double planConfidence = -1.0;           // < 0: not given
    double refineTau = 0.0;                 // 0: not given
    int refineMax = 64;
    float reflect = -1.0f;                  // < 0: not given
    int reflectS = 16;
    int reflectK = 0;                       // 0: not given
    int reflectSided = 0;                   // --reflect-sided
    std::string reflectMapFile;             // --reflect-map
    std::string mirrorMapFile;              // --mirror-map
    std::string sensorsFile, sensorDump;    // --sensors, --sensor-dump
    int sensorSamples = -1;                 // --sensor-samples
    bool calibrateSensor = false;           // --calibrate-sensor P K I
    float calSensorP = 0;
    int calSensorK = 0, calSensorI = 0;
    int gatherBatch = -1;                   // < 0: not given
    std::string verifyDump;
    float calP = 2909.0f, calH = 0.8f, calD = 1.0f;   // userinterface.cpp:107-109 defaults
    ViewMode view = dosage;
    for (int i = 1; i < argc; ++i) {
        auto need = [&](int k) { if (i + k >= argc) { fprintf(stderr, "missing value for %s\n", argv[i]); exit(2); } };
        if (!strcmp(argv[i], "--room")) { need(1); room = argv[++i]; }
        else if (!strcmp(argv[i], "--route-dir")) { need(1); routeDir = argv[++i]; }
        else if (!strcmp(argv[i], "--route")) { need(1); route = argv[++i]; }
        else if (!strcmp(argv[i], "--photons")) { need(1); photons = atoll(argv[++i]); }
        else if (!strcmp(argv[i], "--iterations")) { need(1); iterations = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--lamps")) { need(1); lamps = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--device")) { need(1); device = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--gpus")) { need(1); gpus = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--batch")) { need(1); batch = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--flavour")) { need(1); flavour = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--dump")) { need(1); dump = argv[++i]; }
        else if (!strcmp(argv[i], "--ply")) { need(1); ply = argv[++i]; }
        else if (!strcmp(argv[i], "--save-route")) { need(1); saveRoute = argv[++i]; }
        else if (!strcmp(argv[i], "--view")) { need(1); view = !strcmp(argv[++i], "maxpower") ? maxpower : dosage; }
        else if (!strcmp(argv[i], "--calibrate")) { need(3); calibrate = true; calP = (float)atof(argv[++i]); calH = (float)atof(argv[++i]); calD = (float)atof(argv[++i]); }
        else if (!strcmp(argv[i], "--plan")) {
            plan = true;
            if (i + 1 < argc && strncmp(argv[i + 1], "--", 2) != 0) planMin = (float)atof(argv[++i]);
        }
        else if (!strcmp(argv[i], "--candidates")) {
            need(1);
            const char* v = argv[++i];
            if (strncmp(v, "grid:", 5) != 0 || sscanf(v + 5, "%d,%d,%f", &gridX, &gridZ, &gridInset) < 2 || gridX < 1 || gridZ < 1 ||
                gridX * gridZ > 256) {
                fprintf(stderr, "--candidates grid:NX,NZ[,INSET] (NX x NZ <= 256)\n");
                return 2;
            }
        }
        else if (!strcmp(argv[i], "--drive-speed")) { need(1); driveSpeed = (float)atof(argv[++i]); if (!(driveSpeed >= 0.0f)) { fprintf(stderr, "--drive-speed must be >= 0\n"); return 2; } }
        else if (!strcmp(argv[i], "--plan-drive")) { need(1); plan = true; planDrive = (float)atof(argv[++i]); if (!(planDrive >= 0.0f)) { fprintf(stderr, "--plan-drive must be >= 0\n"); return 2; } }
        else if (!strcmp(argv[i], "--gather")) { need(1); gather = atoi(argv[++i]); if (gather < 0 || gather > 4096) { fprintf(stderr, "--gather must be in [0, 4096]\n"); return 2; } }
        else if (!strcmp(argv[i], "--plan-gather")) { need(1); plan = true; planGather = atoi(argv[++i]); if (planGather < 1 || planGather > 4096) { fprintf(stderr, "--plan-gather must be in [1, 4096]\n"); return 2; } }
        else if (!strcmp(argv[i], "--gather-sampling")) {
            need(1);
            const char* v = argv[++i];
            if (!strcmp(v, "independent")) gatherSampling = UVRT_GATHER_INDEPENDENT;
            else if (!strcmp(v, "stratified")) gatherSampling = UVRT_GATHER_STRATIFIED;
            else { fprintf(stderr, "--gather-sampling independent|stratified (with --gather S or --plan-gather S)\n"); return 2; }
        }
        else if (!strcmp(argv[i], "--plan-confidence")) {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            planConfidence = strtod(v, &end);
            if (end == v || *end != 0 || !std::isfinite(planConfidence) || !(planConfidence >= 0.0)) {
                fprintf(stderr, "--plan-confidence Z: Z must be a finite number >= 0 (with --plan-gather S, S >= 2)\n");
                return 2;
            }
        }
        else if (!strcmp(argv[i], "--gather-refine")) {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            refineTau = strtod(v, &end);
            bool ok = end != v && std::isfinite(refineTau) && refineTau > 0.0;
            if (ok && *end == ',') {
                const char* m = end + 1;
                const long extra = strtol(m, &end, 10);
                ok = end != m && *end == 0 && extra >= 2 && extra <= 4096 && (extra & (extra - 1)) == 0;
                refineMax = (int)extra;
            } else if (ok) {
                ok = *end == 0;
            }
            if (!ok) {
                fprintf(stderr, "--gather-refine TAU[,MAX]: TAU must be a finite number > 0, MAX a power of two in [2, 4096] (with --gather S or --plan-gather S, S >= 2)\n");
                return 2;
            }
        }
        else if (!strcmp(argv[i], "--reflect")) {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            const double rho = strtod(v, &end);
            bool ok = end != v && std::isfinite(rho) && rho >= 0.0 && rho <= 1.0;
            if (ok && *end == ',') {
                const char* m = end + 1;
                const long s2 = strtol(m, &end, 10);
                ok = end != m && *end == 0 && s2 >= 2 && s2 <= 4096 && (s2 & 1) == 0;
                reflectS = (int)s2;
            } else if (ok) {
                ok = *end == 0;
            }
            if (!ok) {
                fprintf(stderr, "--reflect RHO[,S2]: RHO must be in [0, 1], S2 even and in [2, 4096] (with --gather S or --plan-gather S)\n");
                return 2;
            }
            reflect = (float)rho;
        }
        else if (!strcmp(argv[i], "--reflect-bounces")) {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            const long k = strtol(v, &end, 10);
            if (end == v || *end != 0 || k < 1 || k > 16) {
                fprintf(stderr, "--reflect-bounces K: K must be an integer in [1, 16] (with --reflect RHO[,S2])\n");
                return 2;
            }
            reflectK = (int)k;
        }
        else if (!strcmp(argv[i], "--reflect-sided")) reflectSided = 1;
        else if (!strcmp(argv[i], "--reflect-map")) { need(1); reflectMapFile = argv[++i]; if (reflectMapFile.empty() || reflectMapFile.find_first_of("<>&") != std::string::npos) { fprintf(stderr, "--reflect-map FILE: a file name without <, > and & (it goes into route files as it is)\n"); return 2; } }
        else if (!strcmp(argv[i], "--mirror-map")) { need(1); mirrorMapFile = argv[++i]; if (mirrorMapFile.empty() || mirrorMapFile.find_first_of("<>&") != std::string::npos) { fprintf(stderr, "--mirror-map FILE: a file name without <, > and & (it goes into route files as it is)\n"); return 2; } }
        else if (!strcmp(argv[i], "--gather-batch")) {
            need(1);
            char* end = nullptr;
            const char* v = argv[++i];
            const long b = strtol(v, &end, 10);
            if (end == v || *end != 0 || b < 0 || b > UVRT_GATHER_BATCH_MAX) {
                fprintf(stderr, "--gather-batch B: B must be an integer in [0, 64] (with --gather S or --plan-gather S)\n");
                return 2;
            }
            gatherBatch = (int)b;
        }
        else if (!strcmp(argv[i], "--min-photons")) { need(1); minPhotons = atoi(argv[++i]); }
        else if (!strcmp(argv[i], "--plan-verify")) planVerify = true;
        else if (!strcmp(argv[i], "--verify-dump")) { need(1); verifyDump = argv[++i]; }
        else if (!strcmp(argv[i], "--plan-holdout")) { need(1); planHoldout = true; holdoutSeed = (uint32_t)strtoul(argv[++i], nullptr, 0); }
        else if (!strcmp(argv[i], "--sensors")) { need(1); sensorsFile = argv[++i]; if (sensorsFile.empty() || sensorsFile.find_first_of("<>&") != std::string::npos) { fprintf(stderr, "--sensors FILE: a file name without <, > and & (it goes into route files as it is)\n"); return 2; } }
        else if (!strcmp(argv[i], "--sensor-samples")) { need(1); sensorSamples = atoi(argv[++i]); if (sensorSamples < 1 || sensorSamples > 4096) { fprintf(stderr, "--sensor-samples must be in [1, 4096]\n"); return 2; } }
        else if (!strcmp(argv[i], "--sensor-dump")) { need(1); sensorDump = argv[++i]; }
        else if (!strcmp(argv[i], "--calibrate-sensor")) { need(3); calibrateSensor = true; calSensorP = (float)atof(argv[++i]); calSensorK = atoi(argv[++i]); calSensorI = atoi(argv[++i]); }
        else { fprintf(stderr, "unknown option %s\n", argv[i]); return 2; }
    }
    if (room.empty()) { fprintf(stderr, "usage: uvrt_cli --room file.glb [options]\n"); return 2; }
    if (gatherSampling >= 0 && !(gather > 0) && !(planGather > 0)) { fprintf(stderr, "--gather-sampling needs --gather S or --plan-gather S (S > 0)\n"); return 2; }
    if (planConfidence >= 0.0 && planGather < 2) { fprintf(stderr, "--plan-confidence needs --plan-gather S with S >= 2\n"); return 2; }
    if (refineTau > 0.0 && gather < 2 && planGather < 2) { fprintf(stderr, "--gather-refine needs --gather S or --plan-gather S with S >= 2\n"); return 2; }
    if (reflect >= 0.0f && !(gather > 0) && !(planGather > 0)) { fprintf(stderr, "--reflect needs --gather S or --plan-gather S (S > 0)\n"); return 2; }
    if (reflect >= 0.0f && planConfidence >= 0.0) { fprintf(stderr, "--reflect cannot be combined with --plan-confidence (the variance plane knows nothing of the indirect part)\n"); return 2; }
    if (reflectK > 0 && !(reflect >= 0.0f)) { fprintf(stderr, "--reflect-bounces needs --reflect RHO[,S2] (with --gather S or --plan-gather S)\n"); return 2; }
    if (reflectSided && reflectK < 1) { fprintf(stderr, "--reflect-sided needs --reflect-bounces K (with --reflect RHO[,S2]): the traced single bounce has no face-resolved form\n"); return 2; }
    if (reflectSided && !(reflect > 0.0f)) { fprintf(stderr, "--reflect-sided needs --reflect RHO with RHO > 0: without a bounce there are no faces to resolve\n"); return 2; }
    if (reflectSided && gatherBatch >= 2) { fprintf(stderr, "--reflect-sided cannot be combined with --gather-batch B >= 2 (a gather batch keeps no face planes)\n"); return 2; }
    if (!reflectMapFile.empty() && !reflectSided) { fprintf(stderr, "--reflect-map needs --reflect-sided (with --reflect RHO[,S2] and --reflect-bounces K): only the face-resolved bounces know which face a reflectance belongs to\n"); return 2; }
    if (!mirrorMapFile.empty() && !(gather > 0) && !(planGather > 0)) { fprintf(stderr, "--mirror-map needs --gather S or --plan-gather S (S > 0): the mirror gather adds to the direct gather's plane\n"); return 2; }
    if (!mirrorMapFile.empty() && planConfidence >= 0.0) { fprintf(stderr, "--mirror-map cannot be combined with --plan-confidence (the variance plane knows nothing of the specular part)\n"); return 2; }
    if (gatherBatch >= 0 && !(gather > 0) && !(planGather > 0)) { fprintf(stderr, "--gather-batch needs --gather S or --plan-gather S (S > 0)\n"); return 2; }
    if (planGather > 0 && gather > 0) { fprintf(stderr, "--plan-gather cannot be combined with --gather (it plans a route of stops and segments and gathers on its own)\n"); return 2; }
    if (planGather > 0 && batch > 0) { fprintf(stderr, "--plan-gather cannot be combined with --batch (the direct gather runs launch by launch)\n"); return 2; }
    if (planGather > 0 && gpus != 1) { fprintf(stderr, "--plan-gather runs on one context (--gpus 1)\n"); return 2; }
    if (planGather > 0 && planHoldout) { fprintf(stderr, "--plan-gather cannot be combined with --plan-holdout (a gather plan has no holdout seeds)\n"); return 2; }
    if (driveSpeed > 0.0f && plan) { fprintf(stderr, "--drive-speed cannot be combined with --plan (plan a driving route with --plan-drive V)\n"); return 2; }
    if (planDrive > 0.0f && gpus != 1) { fprintf(stderr, "--plan-drive runs on one context (--gpus 1)\n"); return 2; }
    if (driveSpeed > 0.0f && gpus != 1) { fprintf(stderr, "--drive-speed runs on one context (--gpus 1)\n"); return 2; }
    if (gather > 0 && batch > 0) { fprintf(stderr, "--gather cannot be combined with --batch (the direct gather runs launch by launch)\n"); return 2; }
    if (gather > 0 && gpus != 1) { fprintf(stderr, "--gather runs on one context (--gpus 1)\n"); return 2; }
    if (gather > 0 && plan) { fprintf(stderr, "--gather cannot be combined with --plan / --plan-drive (the planner's exposure matrix holds photon counts)\n"); return 2; }
    if (!sensorsFile.empty() && !mirrorMapFile.empty()) { fprintf(stderr, "--sensors cannot be combined with --mirror-map (a sensor would not see the panels' light)\n"); return 2; }
    if (!sensorsFile.empty() && gpus != 1) { fprintf(stderr, "--sensors runs on one context (--gpus 1)\n"); return 2; }
    if (!sensorsFile.empty() && batch > 0) { fprintf(stderr, "--sensors cannot be combined with --batch (the sensors are gathered launch by launch)\n"); return 2; }
    if (!routeDir.empty() && routeDir.back() != '/') routeDir += '/';

    Mesh mesh;
    if (!mesh.LoadMeshFromFile(room.c_str())) return 1;

    RayTracer rayTracer;
    rayTracer.deviceId = device;
    rayTracer.routeDir = routeDir;
    rayTracer.autoSaveRoute = false;
    strncpy(rayTracer.defaultRouteFile, route.c_str(), 31);
    rayTracer.Init(&mesh);                                   // myapp.cpp:39
    if (rayTracer.lightPositions.empty()) rayTracer.AddLamp();
    if (lamps > 0 && lamps < (int)rayTracer.lightPositions.size()) rayTracer.lightPositions.resize(lamps);
    if (photons > 0) rayTracer.photonCount = (int)photons;
    if (iterations > 0) rayTracer.maxIterations = iterations;
    if (driveSpeed >= 0.0f) rayTracer.driveSpeed = driveSpeed;
    if (planDrive >= 0.0f) rayTracer.driveSpeed = planDrive;
    if (rayTracer.driveSpeed > 0.0f && gpus != 1) {               // (the route file's own <rijsnelheid>)
        fprintf(stderr, "the route drives at %g m/s: not supported with --gpus > 1 (give --drive-speed 0)\n", (double)rayTracer.driveSpeed);
        return 2;
    }
    if (gather >= 0) rayTracer.gatherSamples = gather;
    if (gatherSampling >= 0 && gather > 0) rayTracer.gatherSampling = gatherSampling;
    if (refineTau > 0.0 && gather > 0) { rayTracer.gatherRelError = refineTau; rayTracer.gatherMaxExtra = refineMax; }
    if (reflect >= 0.0f && gather > 0) { rayTracer.reflectance = reflect; rayTracer.reflectSamples = reflectS; rayTracer.reflectBounces = reflectK; rayTracer.reflectSided = reflectSided; rayTracer.reflectMap = reflectMapFile; }
    if (gatherBatch >= 0) rayTracer.gatherBatch = gatherBatch;
    if (!mirrorMapFile.empty()) rayTracer.mirrorMap = mirrorMapFile;
    else if (rayTracer.gatherSamples == 0 || plan) rayTracer.mirrorMap.clear();    // (the route file's own <mirror_map>: a plan's panels are --mirror-map's)
    if (rayTracer.gatherSamples == 0 || plan) rayTracer.reflectance = 0.0f;    // (the route file's own <reflectance>: a plan's bounce is --reflect's)
    if (rayTracer.gatherSamples == 0 || plan) rayTracer.reflectMap = planGather > 0 ? reflectMapFile : std::string();   // (likewise its <reflect_map>)
    if (rayTracer.gatherSamples > 0 && (batch > 0 || gpus != 1 || plan)) {     // (the route file's own <gather_samples>)
        fprintf(stderr, "the route gathers with %d samples: not supported with --batch, --gpus > 1 or --plan (give --gather 0)\n", rayTracer.gatherSamples);
        return 2;
    }
    if (!sensorsFile.empty()) rayTracer.sensorMap = sensorsFile;
    else if (batch > 0 || gpus != 1 || plan) rayTracer.sensorMap.clear();      // (the route file's own <sensor_map>)
    if (sensorSamples > 0) rayTracer.sensorSamples = sensorSamples;
    if (rayTracer.HasSensors() && rayTracer.HasMirrors()) {
        fprintf(stderr, "sensors cannot be combined with mirror panels (a sensor would not see the panels' light)\n");
        return 2;
    }
    if ((calibrateSensor || !sensorDump.empty() || sensorSamples > 0) && !rayTracer.HasSensors()) {
        fprintf(stderr, "--sensor-samples, --sensor-dump and --calibrate-sensor need --sensors FILE\n");
        return 2;
    }
    if (rayTracer.HasSensors()) {
        const std::string err = rayTracer.PrepareSensorMap();
        if (!err.empty()) { fprintf(stderr, "--sensors: %s\n", err.c_str()); return 2; }
        if (calibrateSensor && (calSensorK < 0 || (size_t)calSensorK >= rayTracer.ActiveSensors().size() || calSensorI < 0 ||
                                (size_t)calSensorI >= rayTracer.lightPositions.size())) {
            fprintf(stderr, "--calibrate-sensor P K I: sensor K of %zu, lamp position I of %zu\n", rayTracer.ActiveSensors().size(),
                    rayTracer.lightPositions.size());
            return 2;
        }
    }
    rayTracer.UpdatePhotonsPerLight();

    if (calibrate) {
        rayTracer.CalibratePower(calP, calH, calD);          // userinterface.cpp:130-133
        std::cout << "Calibrated lamp power: " << rayTracer.lightIntensity << std::endl;
    }

    if (calibrateSensor) {
        if (uvrt_set_flavour(rayTracer.ctx, flavour) != UVRT_OK) { fprintf(stderr, "--flavour: %s\n", uvrt_last_error()); return 2; }
        rayTracer.CalibratePowerAtSensor(calSensorP, calSensorK, calSensorI);
        std::cout << "Calibrated lamp power at sensor " << calSensorK << ": " << rayTracer.lightIntensity << std::endl;
    }

    if (plan) {
        if (gpus != 1) { fprintf(stderr, "--plan runs on one context (--gpus 1)\n"); return 2; }
        if (uvrt_set_flavour(rayTracer.ctx, flavour) != UVRT_OK) { fprintf(stderr, "--flavour: %s\n", uvrt_last_error()); return 2; }
        if (gridX > 0) rayTracer.SetCandidateGrid(gridX, gridZ, gridInset);
        if (rayTracer.driveSpeed > 0.0f && rayTracer.lightPositions.size() > 128) {
            fprintf(stderr, "a driving plan takes at most 128 positions (%zu given)\n", rayTracer.lightPositions.size());
            return 2;
        }
        rayTracer.ResetDosageMap();
        rayTracer.viewMode = dosage;
        const int rc = run_plan(rayTracer, planMin, minPhotons, planVerify, planHoldout, holdoutSeed, batch, dump, verifyDump, planGather,
                                gatherSampling < 0 ? 0 : gatherSampling, planConfidence < 0.0 ? 0.0 : planConfidence, refineTau, refineMax,
                                reflect < 0.0f ? 0.0f : reflect, reflectS, reflectK, reflectSided, reflectMapFile.empty() ? 0 : 1,
                                mirrorMapFile.empty() ? 0 : 1);
        save_route(rayTracer, saveRoute);
        return rc;
    }
    // --gpus N: further instances of the same RayTracer, one per context, each with its range of every launch
    std::vector<RayTracer*> group{&rayTracer};
    std::vector<RayTracer*> extra;
    if (gpus < 1 || gpus > 64) { fprintf(stderr, "--gpus must be in [1,64]\n"); return 2; }
    if (gpus > 1) {
        const int ndev = uvrt_device_count();
        if (batch <= 0) batch = 1;
        for (int r = 1; r < gpus; ++r) {
            RayTracer* rt = new RayTracer();
            rt->deviceId = ndev >= gpus ? device + r : device;
            rt->routeDir = routeDir;
            rt->autoSaveRoute = false;
            strncpy(rt->defaultRouteFile, route.c_str(), 31);
            rt->Init(&mesh);
            rt->lightPositions = rayTracer.lightPositions;
            rt->photonCount = rayTracer.photonCount;
            rt->maxIterations = rayTracer.maxIterations;
            rt->lightIntensity = rayTracer.lightIntensity;
            rt->UpdatePhotonsPerLight();
            extra.push_back(rt);
            group.push_back(rt);
        }
        if (ndev >= gpus) {
            std::vector<uvrt_ctx*> ctxs;
            for (RayTracer* rt : group) ctxs.push_back(rt->ctx);
            if (uvrt_comm_init_all(ctxs.data(), gpus) != UVRT_OK) { fprintf(stderr, "comm_init_all: %s\n", uvrt_last_error()); return 1; }
            std::cout << "Sharding every launch over " << gpus << " GPUs, one RCCL all-reduce of the count planes per batch" << std::endl;
        } else {
            std::cout << "Sharding every launch over " << gpus << " contexts on " << ndev << " GPU(s) (rehearsal: no RCCL)" << std::endl;
        }
    }
    for (size_t r = 0; r < group.size(); ++r) {
        if (uvrt_set_flavour(group[r]->ctx, flavour) != UVRT_OK) { fprintf(stderr, "--flavour: %s\n", uvrt_last_error()); return 2; }
        group[r]->ResetDosageMap();                          // userinterface.cpp:247-251
        group[r]->viewMode = view;
        if (gpus > 1) group[r]->SetRayRange((int)r, gpus);
    }
    while (!rayTracer.finishedComputation) {                 // myapp.cpp:156-175
        rayTracer.finishedComputation = rayTracer.currIterations >= rayTracer.maxIterations;
        if (rayTracer.finishedComputation) break;
        if (batch > 0) {
            RayTracer::ComputeIterationsBatched(group, std::min(batch, rayTracer.maxIterations - rayTracer.currIterations));
        } else {
            rayTracer.ComputeDosageMap();
            rayTracer.Shade();
            rayTracer.currIterations++;
        }
        if (rayTracer.viewMode == texture) rayTracer.viewMode = dosage;
        rayTracer.progress = 100.0f * static_cast<float>(rayTracer.currIterations) / static_cast<float>(rayTracer.maxIterations);
        for (RayTracer* rt : group) rt->Sync();
        float time = rayTracer.timerClock.elapsed();
        rayTracer.compTime += time;
        std::cout << "Progress: " << rayTracer.progress << "% photon count: " << rayTracer.photonMapSize
                  << " delta time: " << time * 1000.0f << " total time: " << rayTracer.compTime * 1000.0f << std::endl;
        rayTracer.timerClock.reset();
    }
    const double rays = (double)rayTracer.photonMapSize;
    std::cout << "Traced " << rays << " photons in " << rayTracer.compTime * 1000.0f << " ms = "
              << rays / rayTracer.compTime / 1e6 << " Mray/s" << std::endl;

    std::vector<float> dose(mesh.triangleCount);
    rayTracer.ReadDosage(dose.data(), 0, mesh.triangleCount);
    double sum = 0;
    int nonzero = 0;
    for (float d : dose) { sum += d; nonzero += d != 0.0f; }
    printf("dose: sum %.6f, %d of %d triangles non-zero, dose[0..3] = %.9g %.9g %.9g %.9g\n", sum, nonzero,
           mesh.triangleCount, dose[0], dose.size() > 1 ? dose[1] : 0.f, dose.size() > 2 ? dose[2] : 0.f,
           dose.size() > 3 ? dose[3] : 0.f);
    if (!dump.empty()) write_f32(dump, dose);
    if (rayTracer.HasSensors()) {
        std::vector<float> sdose, speak;
        std::vector<double> serr;
        rayTracer.ReadSensors(sdose, speak, serr);
        const std::vector<uvrt_sensor>& sens = rayTracer.ActiveSensors();
        printf("sensors: %zu, dose[0] = %.9g mJ/cm^2, peak[0] = %.9g uW/cm^2\n", sens.size(), sdose[0], speak[0]);
        if (!sensorDump.empty()) {
            FILE* f = fopen(sensorDump.c_str(), "w");
            if (!f) { fprintf(stderr, "--sensor-dump: cannot write %s\n", sensorDump.c_str()); return 1; }
            fprintf(f, "index,kind,x,y,z,nx,ny,nz,dose,peak,std_err\n");
            for (size_t k = 0; k < sens.size(); ++k)
                fprintf(f, "%zu,%s,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.9g,%.17g\n", k, sens[k].kind == UVRT_SENSOR_PLANAR ? "planar" : "sphere",
                        sens[k].pos[0], sens[k].pos[1], sens[k].pos[2], sens[k].normal[0], sens[k].normal[1], sens[k].normal[2], sdose[k],
                        speak[k], serr[k]);
            fclose(f);
        }
    }
    if (!ply.empty()) {
        std::vector<float> color((size_t)mesh.triangleCount * 9);
        if (uvrt_read_color(rayTracer.ctx, color.data(), 0, mesh.triangleCount) != UVRT_OK) {
            fprintf(stderr, "read_color: %s\n", uvrt_last_error());
            return 1;
        }
        std::ofstream f(ply, std::ios::binary);
        f << "ply\nformat binary_little_endian 1.0\ncomment UV dose heat map (dosageToColor)\n"
          << "element vertex " << mesh.triangleCount * 3 << "\nproperty float x\nproperty float y\nproperty float z\n"
          << "property uchar red\nproperty uchar green\nproperty uchar blue\n"
          << "element face " << mesh.triangleCount << "\nproperty list uchar int vertex_indices\nend_header\n";
        auto to8 = [](float v) { v = v < 0 ? 0 : (v > 1 ? 1 : v); return (unsigned char)(v * 255.0f + 0.5f); };
        for (int i = 0; i < mesh.triangleCount; ++i)
            for (int k = 0; k < 3; ++k) {
                f.write((const char*)(mesh.vertices + (size_t)i * 9 + k * 3), 12);
                const unsigned char rgb[3] = {to8(color[(size_t)i * 9 + k * 3]), to8(color[(size_t)i * 9 + k * 3 + 1]),
                                              to8(color[(size_t)i * 9 + k * 3 + 2])};
                f.write((const char*)rgb, 3);
            }
        for (int i = 0; i < mesh.triangleCount; ++i) {
            const unsigned char three = 3;
            const int idx[3] = {3 * i, 3 * i + 1, 3 * i + 2};
            f.write((const char*)&three, 1);
            f.write((const char*)idx, 12);
        }
    }
    for (RayTracer* rt : extra) {
        // every instance holds the same maps after the reduction: check it, then drop the helpers
        std::vector<float> other(mesh.triangleCount);
        rt->ReadDosage(other.data(), 0, mesh.triangleCount);
        if (memcmp(other.data(), dose.data(), dose.size() * 4) != 0) { fprintf(stderr, "rank doses differ\n"); return 1; }
        delete rt;
    }
    save_route(rayTracer, saveRoute);                        // myapp.cpp:298
    return 0;
}

// raytracer.h -- host mirror of the reference's RayTracer (raytracer.h:5-59): same class
// name, namespace, method signatures and public data members, so MyApp / UserInterface code
// written against the reference drives this one unchanged.  The OpenCL `Kernel*` / `Buffer*`
// members are replaced by one opaque uvrt_ctx (include/uvrt.h); everything else is kept.
#pragma once
#include "template_types.h"
#include "mesh.h"
#include "../../include/uvrt.h"

#include <string>
#include <vector>

struct uvrt_ctx;

namespace Tmpl8 {

struct LightPos {              // raytracer.h:5-9
    float2 position;
    float duration;
};

enum ViewMode { dosage, maxpower, texture };   // raytracer.h:11

// one launch of an iteration of a route (RayTracer::RouteLaunches); `to` is all zero at a stop
struct RouteLaunch {
    float from[3], to[3];
    float duration;
    int kind;                  // UVRT_LAUNCH_STOP / UVRT_LAUNCH_SWEEP
    int column;
    int reserved;              // 0: the record is 40 bytes (uvrt_host_route_launches)
};

class RayTracer {
public:
    RayTracer() = default;
    ~RayTracer();
    RayTracer(const RayTracer&) = delete;
    RayTracer& operator=(const RayTracer&) = delete;

    void Init(Mesh* mesh);                                   // raytracer.cpp:12-59
    void UpdatePhotonsPerLight();                            // :61-64
    void ComputeDosageMap();                                 // :66-72
    void ComputeSingleLightDosageMap(LightPos lightPos, int photonsPerLight, int triangleCount);   // :75-88
    void Shade();                                            // :93-120
    void ResetDosageMap();                                   // :122-131
    void ClearBuffers(bool resetColor);                      // :133-143
    void AddLamp();                                          // :3-10
    void CalibratePower(float measurePower, float measureHeight, float measureDist);   // :151-227
    void SaveRoute(char fileName[32]);                       // :233-259
    void LoadRoute(char fileName[32]);                       // :261-300

    float lightLength = 1.0f;
    float lightHeight = 0.8f;
    int maxPhotonCount = (1 << 26);
    int photonCount = (1 << 25);
    int maxIterations = 10;
    int currIterations = 0;   // The number of computed iterations
    float lightIntensity = 450;
    float minDosage = 100, minPower = 1500;
    char defaultRouteFile[32] = "route";
    char newRouteFile[32] = "new_route";

    Mesh* mesh = nullptr;
    float* dosageMap = new float[2];
    std::vector<LightPos> lightPositions;
    int photonsPerLight = 0;   // The number of photons per light of a single iteration
    float compTime = 0;
    float progressTextTimer = 0;
    float progress = 0;
    Timer timerClock;
    bool finishedComputation = true;
    ViewMode viewMode = texture;
    bool thresholdView = false;
    bool startedComputation = false;
    float calibratedPower = 0;
    int photonMapSize = 0;
    void* simpleShader = nullptr;   // ShaderGL* in the reference; not used by the compute path

    // ---- additions of the headless build (not in the reference) ----
    uvrt_ctx* ctx = nullptr;            // replaces the six Kernel* and nine Buffer* members
    int deviceId = 0;                   // HIP device the context is created on
    std::string routeDir = "positions/";   // prefix of SaveRoute/LoadRoute (raytracer.cpp:257,263)
    bool autoSaveRoute = true;          // ResetDosageMap rewrites positions/route.xml (:126)
    // Multi-GPU launch sharding (DESIGN.md "Multi-GPU"): of the global sequence of lamp launches
    // (every ComputeSingleLightDosageMap call, in order) this instance runs those with
    // index % shardWorld == shardRank and only advances the SEED chain for the others, so the
    // union over ranks is the single-GPU computation.  The owner of the ranks then reduces
    // photonMap with SUM and maxPhotonMap with MAX (both exact) before Shade().
    int shardRank = 0, shardWorld = 1;
    long long launchIndex = 0;
    // Batched computation (include/uvrt.h "batched tracing"): what MyApp::Tick does over `iterations`
    // frames (myapp.cpp:156-163: ComputeDosageMap(); Shade(); currIterations++), with all launches of a
    // batch traced first and accumulate + Shade replayed per launch afterwards: same maps, dose and colours
    // bit for bit, far fewer kernel launches.  `group`: instances that together trace every launch by
    // global-id range (rangeFirst / rangeCount; BASELINE configs[3] "pixel tiles") inside ONE process --
    // their planes are summed by uvrt_reduce_batch_group; an instance whose context holds a communicator
    // (one process per GPU, uvrt_comm_init_rank) reduces over it.
    void ComputeIterationsBatched(int iterations);
    static void ComputeIterationsBatched(const std::vector<RayTracer*>& group, int iterations);
    long long rangeFirst = 0, rangeCount = -1;      // -1: the whole launch
    bool reduceOverComm = false;                    // ctx has a communicator: all-reduce the planes of every batch
    void SetRayRange(int rank, int world);          // contiguous share of [0, photonsPerLight) for rank of world
    // Duration planning (include/uvrt.h "duration planning"): one batched computation over the current
    // lightPositions from the current SEED with the exposure captured, the covering LP solved, and the least
    // durations that bring every required triangle to minDose written into lightPositions (positions the plan
    // does not need keep their place with duration 0, so a recompute traces the same rays).  `group`: instances
    // that share every launch by ray range; every context captures after the group reduce and solves on its own
    // (identical durations).  minDose < 0: the route's minDosage.  Returns the solver's report; *seedOut is the
    // SEED the computation started from.
    struct PlanOptions {
        float minDose = -1.0f;
        int minPhotons = 16;
        double margin = 1e-6, relGap = 1e-3;
        int maxIterations = 200;       // cutting-plane rounds of the solver
        const unsigned char* mask = nullptr;    // uint8[T], 0 = not required
        // S > 0: plan from the direct gather (include/uvrt.h "planning from the direct gather"): on this one context, the
        // launches ComputeDosageMap runs with gatherSamples = S for maxIterations iterations (seed = the launch counter from 0,
        // Shade after every iteration), every plane captured into its launch's column of an exposure matrix of f64 expected
        // counts; columns, bounds and N = maxIterations x photonsPerLight as for a counts plan.  A group of more than one
        // instance, shardWorld > 1 and reduceOverComm are fatal.  0: photon counts (RayTracer::gatherSamples > 0 is fatal).
        int gatherSamples = 0;
        // the gather sampling mode of those launches (uvrt_set_gather_sampling; read only with gatherSamples > 0).  Like S it
        // is the plan's own: RayTracer::gatherSampling is not touched.
        int gatherSampling = 0;
        // z > 0: plan for the lower confidence bound of the gather's estimate (include/uvrt.h "planning for a lower confidence
        // bound"): the same launches with the variance plane on, an exposure matrix with its variance, and
        // uvrt_plan_lower_confidence(z) before the solve -- every required triangle reaches the minimum for expected - z
        // standard errors, element by element.  The context's variance state is put back afterwards; no public field is
        // touched.  0 (default): the plan above, bit for bit.  Not 0 with gatherSamples < 2, negative or not finite: fatal.
        // Meant for gatherSamples >= 16: at 4 samples about half the bounds are 0.
        double gatherConfidence = 0.0;
        // tau > 0: every gather launch of the plan is refined before its capture (RayTracer::gatherRelError below, with
        // gatherMaxExtra beside it), with and without gatherConfidence.  The plan's own, like S: the RayTracer members are not
        // touched.  0 (default): the plan above, bit for bit.  Not 0 with gatherSamples < 2, negative or not finite: fatal.
        double gatherRelError = 0.0;
        int gatherMaxExtra = 64;
        // rho > 0: every gather launch of the plan gets one diffuse bounce before its capture (RayTracer::reflectance below,
        // with reflectSamples beside it).  The plan's own, like S.  0 (default): the plan above, bit for bit.  Not 0 with
        // gatherSamples = 0, outside [0, 1], or with gatherConfidence != 0: fatal -- the variance plane knows nothing of the
        // indirect part, so the bound would promise more than it has.
        float reflectance = 0.0f;
        int reflectSamples = 16;
        // K in [1, 16] with reflectance > 0: the plan's launches take K bounces over recorded hit links instead of the traced
        // one (RayTracer::reflectBounces below).  0 (default): the traced bounce, bit for bit.  Outside [0, 16]: fatal.
        int reflectBounces = 0;
        // 1 with reflectance > 0 and reflectBounces >= 1: the plan's bounces are face-resolved (RayTracer::reflectSided below).
        // 0 (default): the two-sided bounces, bit for bit.  1 with reflectance 0, reflectBounces 0 or gatherBatch >= 2: fatal.
        int reflectSided = 0;
        // 1 with reflectSided = 1: the plan's bounces take the ray tracer's reflectance map (RayTracer::reflectMap or
        // SetReflectanceMap below) in place of the one rho.  0 (default): the plan above, bit for bit.  1 without reflectSided or
        // without a map: fatal.
        int reflectMapped = 0;
        // 1 with gatherSamples > 0: every gather launch of the plan is followed by the mirror gather over the ray tracer's
        // specular panels (RayTracer::mirrorMap or SetMirrors below).  0 (default): the plan above, bit for bit.  1 without
        // panels, without gatherSamples or with gatherConfidence != 0 (the variance plane is the direct part's): fatal.
        int mirrorMapped = 0;
        // B in [2, 64]: the plan's gather launches are traced in groups of up to B (RayTracer::gatherBatch below).  The plan's
        // own, like S.  0 (default) and 1: launch by launch.  Durations, report and every captured column are the same bits
        // for every B.  Outside [0, 64]: fatal.
        int gatherBatch = 0;
    };
    uvrt_plan_report PlanDurations(const PlanOptions& opt, unsigned* seedOut = nullptr);
    static uvrt_plan_report PlanDurations(const std::vector<RayTracer*>& group, const PlanOptions& opt, unsigned* seedOut = nullptr);
    // E (positions x triangles x 4 bytes) stays on the device after PlanDurations, for uvrt_plan_model_dose /
    // uvrt_plan_read_required; EndPlan releases it (so do a new scene and the destructor)
    void EndPlan();
    // replaces lightPositions by an nx x nz grid over the mesh's x/z bounds inset by `inset` metres (duration 1)
    void SetCandidateGrid(int nx, int nz, float inset);
    static void GridPositions(float xmin, float xmax, float zmin, float zmax, int nx, int nz, float inset, float* xz);
    bool planCapture = false;                       // ComputeIterationsBatched captures every batch (PlanDurations)
    // Planning a route that drives (RouteLaunches has segments; at most 128 positions): E has one column per launch, and
    // uvrt_plan_solve_bounded plans the stops (free, lower bound 0) with every segment FIXED at its launch's duration: the
    // plan counts what the drive delivers and says which rows only the drive reaches.  planBounds is that solve's bounds
    // report (met_by_lower: rows the drive alone brings to the minimum; short_rows: rows no stop reaches and the drive
    // leaves below it) and planSegmentDurations the segment columns as solved (= the list's, bit for bit, or fatal); after
    // a plan without driving: no fixed column, L free ones, no segment.
    uvrt_plan_bounds_report planBounds{};
    std::vector<float> planSegmentDurations;
    // Dose while the robot drives.  driveSpeed (m/s) > 0: after the stops of an iteration come the segments between
    // consecutive positions, the lamp radiating while it moves at that speed (include/uvrt.h uvrt_generate_sweep:
    // photonsPerLight photons spread uniformly in time over the segment).  A segment adds its counts with the time the drive
    // takes, like a stop that stood so long, but NOT to photonMapSize: Shade's divisor photonMapSize / lightPositions.size()
    // stays the photons per source.  The maximum map takes a segment's counts like any launch: there it means the mean
    // irradiance over the segment.  0 (default) is the reference's behaviour, bit for bit.  Saved as <rijsnelheid> in route
    // files when > 0.  A group of instances, a ray range and reduceOverComm work with driving as they do without,
    // PlanDurations included; launch sharding (shardWorld > 1) refuses it.
    float driveSpeed = 0;
    // The launches of one iteration, in order; ComputeDosageMap, ComputeIterationsBatched and PlanDurations all walk this
    // one list.  The L stops: from = {x, y, z}, the position's own duration, column i.  Then, iff driveSpeed > 0 (NaN and
    // negative: no) and L >= 2, the L - 1 segments k -> k+1: from and to at the same y, duration len / driveSpeed with len =
    // sqrtf(dx*dx + dz*dz) in f32, column L + k (a zero-length segment is traced too, with duration 0: the SEED chain stays
    // regular).  y is the lamp's foot, the caller's single f32 sum mesh->floorHeight + lightHeight (raytracer.cpp:77).
    static std::vector<RouteLaunch> RouteLaunches(const std::vector<LightPos>& positions, float y, float driveSpeed);
    // one segment: a and b are two positions (their durations are not used)
    void ComputeSegmentDosageMap(LightPos a, LightPos b, int photonsPerLight, int triangleCount);
    void ComputeSegments();                         // the segments of one iteration, in order (nothing at driveSpeed 0)
    // The direct gather in place of photon counting (include/uvrt.h "shadow rays and the direct gather").  gatherSamples
    // = S > 0: every stop of ComputeDosageMap is uvrt_gather_direct over all triangles (S samples each, photons_equiv =
    // photonsPerLight, seed = the number of gather launches since ResetDosageMap) followed by
    // uvrt_accumulate_expected(duration) instead of generate -> extend -> accumulate; photonMapSize advances as before, so
    // Shade is unchanged.  ComputeSegmentDosageMap does the same with from != to (and photonMapSize stays, as with
    // photons).  0 (default) is the reference's behaviour, bit for bit.  Saved as <gather_samples> in route files when
    // > 0.  ComputeIterationsBatched, launch sharding (shardWorld > 1) and PlanDurations refuse it: the gather runs per
    // launch, on one context, and a counts plan's exposure matrix holds photon counts.  To plan from the gather leave this
    // at 0 and give PlanOptions::gatherSamples: the plan is then as good as the estimator.
    int gatherSamples = 0;
    // How the gather places its samples on the lamp (include/uvrt.h uvrt_set_gather_sampling): 0 independent draws (default),
    // 1 rod strata and a rotated sweep sequence.  Handed to the context before every gather launch; read by
    // nothing else.  Saved as <gather_sampling> after <gather_samples> in route files when both are > 0.
    int gatherSampling = 0;
    // The adaptive gather (include/uvrt.h "adaptive gather").  gatherRelError = tau > 0 with gatherSamples >= 2:
    // every gather launch runs with the variance plane on (the context's state is put back after the launch) and is followed
    // by uvrt_gather_refine(rel_error = tau, min_expected = 0, max_extra = gatherMaxExtra, seed = ~the launch's seed) before
    // its plane is captured or accumulated.  0 (default): the gather above, bit for bit.  tau not 0 with gatherSamples < 2
    // (photon launches included), tau negative or not finite: fatal.  Not saved in route files.
    double gatherRelError = 0.0;
    int gatherMaxExtra = 64;
    // One diffuse bounce on top of the direct gather (include/uvrt.h "one diffuse bounce").  reflectance = rho
    // in (0, 1] with gatherSamples > 0: after a launch's gather (and its refine, if any) and before its plane is captured or
    // accumulated, uvrt_indirect_source_from_expected and uvrt_gather_indirect(rho, samples = reflectSamples, seed = the
    // launch's gather seed ^ 0x85EBCA6B, add = 1) over all triangles.  0 (default): the gather above, bit for bit.  rho not 0
    // with gatherSamples = 0, or outside [0, 1]: fatal.  One bounce, one rho for the whole scene; the variance plane stays the
    // direct part's.  Saved as <reflectance> and <reflect_samples> after the gather tags in route files when rho > 0.
    float reflectance = 0.0f;
    int reflectSamples = 16;
    // Bounces over recorded hit links (include/uvrt.h "recorded hit links").  0 (default): the traced bounce
    // above, once per launch, bit for bit.  K in [1, 16] with reflectance > 0: the links are built once per scene
    // (uvrt_indirect_links_build with samples = reflectSamples and the fixed seed 0x85EBCA6B; rebuilt when
    // uvrt_indirect_links_info reports another scene's or another sample count's), and every gather launch does
    // uvrt_indirect_source_from_expected and uvrt_gather_indirect_linked(rho, K, add = 1) over all triangles in place of the
    // traced bounce: no ray is traced per launch, and bounces 2..K come with it.  Every launch then sees the same directions,
    // so the bounce's sampling error no longer averages out over a route; reflectSamples is paid once and can be much larger.
    // Outside [0, 16]: fatal.  Without effect at reflectance 0.  Saved as <reflect_bounces> after <reflect_samples> when both
    // rho and K are > 0.
    int reflectBounces = 0;
    // Face-resolved bounces (include/uvrt.h "face-resolved gather and bounces"): every triangle an opaque sheet
    // whose two faces keep their own irradiance, so that the bounces conserve energy at every reflectance.  1 with reflectance
    // > 0 and reflectBounces = K >= 1: every gather launch runs with the context's faces state on (put back after the launch; a
    // refine may follow, the face planes then describe the first pass), the links are built with
    // uvrt_indirect_links_build_sided (rebuilt when uvrt_indirect_links_info reports another sample count, seed or kind), and
    // uvrt_gather_indirect_linked_sided(rho, K, add = 1) stands where the snapshot and the two-sided call stood.  0 (default):
    // the bounces above, bit for bit.  1 is fatal with reflectance 0 (there is no bounce to resolve), with reflectBounces 0 (the
    // traced single bounce has no face-resolved form) and with gatherBatch >= 2 (a gather batch keeps no face planes).  Saved
    // as <reflect_sided>1</reflect_sided> after <reflect_bounces> when that tag is written and this is on.
    int reflectSided = 0;
    // A reflectance per face in place of the one rho of the face-resolved bounces (include/uvrt.h "per-face reflectance", DESIGN.md
    // 22).  reflectMap names a rules file (empty: none; a relative name is resolved against routeDir):
    //     box X0 Y0 Z0 X1 Y1 Z1 RHO                    both faces of every triangle whose Tri.centroid lies in the closed box
    //     box X0 Y0 Z0 X1 Y1 Z1 RHO toward PX PY PZ    only the face that looks at P
    // (ParseReflectRules below).  Every entry starts at `reflectance`; later lines override earlier ones.  The file is read by the
    // first gather launch that needs it (or by PrepareReflectMap), once per file name and base, into a cache of its own.
    // SetReflectanceMap hands over 2 x triangleCount values directly (face 0's plane, then face 1's) for a caller that brings
    // planes: they are reflectMapValues, and an empty call (nullptr, 0) forgets them.  A file, when one is named, goes before the
    // caller's planes; clearing the name (or loading a route without the tag) leaves no trace of the file: the caller's planes
    // count again, or there is no map.  With a map and reflectSided = 1 every gather launch uploads the planes when
    // uvrt_reflectance_info says the context has none (a scene swap drops them) or the map is not the one uploaded last, and
    // calls uvrt_gather_indirect_linked_mapped(K, add = 1) where uvrt_gather_indirect_linked_sided stood; everything else about
    // the launch stays.  A map without reflectSided and a map whose size is not 2 x triangleCount are fatal.  No map: every path
    // bit for bit as before.  Saved as <reflect_map>FILE</reflect_map> after <reflect_sided> when that tag is written and a
    // file is named; a name that holds <, > or & cannot stand in a route file and is fatal there.
    std::string reflectMap;
    std::vector<float> reflectMapValues;            // the caller's planes (SetReflectanceMap); never the file's
    void SetReflectanceMap(const float* rho2T, int count);
    bool HasReflectanceMap() const { return !reflectMap.empty() || !reflectMapValues.empty(); }
    // Reads reflectMap's file with `base` as every entry's start unless that is what the cache holds; nothing to do without a
    // file name.  Returns an empty string or ParseReflectRules' message: for a caller that wants to hear of a bad file before a
    // launch ends the process over it.
    std::string PrepareReflectMap(float base);
    // the planes a mapped launch would upload now: the file's when a file is named (empty until it has been read), else the
    // caller's
    const std::vector<float>& ActiveReflectanceMap() const;
    // The rules file above into out[2 * triangleCount] (plane-major), every entry starting at `base`.  Host only.  Returns an
    // empty string, or what is wrong as "FILE:LINE: reason": an unknown keyword, a wrong count of numbers, an RHO that is not
    // finite or not in [0, 1], a box with a lower bound above its upper bound (or "FILE: cannot be read").  In a box the
    // centroid is compared in f32, bounds included; `toward P` takes face 0 iff n.(P - v0) > 0 with n = cross(e1, e2), all in
    // f64 from the f32 values, and leaves a triangle with |n| == 0 as it is.
    static std::string ParseReflectRules(const char* path, const Tri* tris, int triangleCount, float base, float* out);
    // Specular panels (include/uvrt.h "specular panels").  mirrorMap names a rules file (empty: none; a relative
    // name is resolved against routeDir, as reflectMap's):
    //     mirror X0 Y0 Z0 X1 Y1 Z1 RHO plane QX QY QZ MX MY MZ
    // Every line makes the next panel: the plane through Q with normal M (it reflects on the side M points to), specular
    // reflectance RHO, its members the triangles whose Tri.centroid lies in the closed box (ParseMirrorRules below; a later
    // line takes a triangle over).  SetMirrors hands panels and panel_of_tri[triangleCount] over directly; an empty call
    // (nullptr, 0, nullptr, 0) forgets them; a file, when one is named, goes before them.  With panels and gatherSamples > 0
    // every gather launch -- after its direct gather (or uvrt_gather_batch_select) and its refine, before its bounces, its
    // capture and its accumulate -- uploads the panels when uvrt_mirror_info says the context has none (a scene swap drops
    // them) or the active panels are not the ones uploaded last, and calls uvrt_gather_mirror(the launch's gather parameters,
    // add = 1) over all triangles, with the faces state on under reflectSided so that the bounces see the specular light.
    // Panels with gatherSamples = 0 and a panel_of_tri whose size is not triangleCount are fatal.  No panels: every path bit
    // for bit as before.  Saved as <mirror_map>FILE</mirror_map>, the last gather tag, when a file is named; a name that
    // holds <, > or & cannot stand in a route file and is fatal there.
    std::string mirrorMap;
    std::vector<uvrt_mirror> mirrorPanels;          // the caller's panels (SetMirrors); never the file's
    std::vector<uint8_t> mirrorPanelOfTri;
    void SetMirrors(const uvrt_mirror* panels, int count, const uint8_t* panelOfTri, int triangleCount);
    bool HasMirrors() const { return !mirrorMap.empty() || !mirrorPanels.empty(); }
    // Reads mirrorMap's file unless that is what the cache holds; nothing to do without a file name.  Returns an empty string
    // or ParseMirrorRules' message.
    std::string PrepareMirrorMap();
    // The rules file above into panelsOut[UVRT_MIRROR_MAX], *countOut and panelOfTriOut[triangleCount] (0 or k + 1).  Host
    // only.  Returns an empty string, or what is wrong as "FILE:LINE: reason": an unknown keyword, a wrong count of numbers, a
    // ninth panel, an RHO that is not finite or not in [0, 1], a zero normal, a value that is not finite where the context
    // would refuse it, a box with a lower bound above its upper bound (or "FILE: cannot be read").  The centroid is compared
    // in f32, bounds included.
    static std::string ParseMirrorRules(const char* path, const Tri* tris, int triangleCount, uvrt_mirror* panelsOut, int* countOut,
                                        uint8_t* panelOfTriOut);
    // Virtual dosimeters (include/uvrt.h "sensors"): dose and fluence at points off the mesh.  sensorMap names a
    // rules file (empty: none; a relative name is resolved against routeDir, as mirrorMap's):
    //     sensor X Y Z planar NX NY NZ                         a one-sided receiver; the side (NX, NY, NZ) points to is sensitive
    //     sensor X Y Z sphere                                  a spherical receiver: fluence rate
    //     grid X0 Y0 Z0 X1 Y1 Z1 NX NY NZ sphere               the cell centres of an NX x NY x NZ lattice over the box, x fastest,
    //     grid X0 Y0 Z0 X1 Y1 Z1 NX NY NZ planar MX MY MZ      then y, then z: X0 + (X1 - X0) * ((i + 0.5f) / NX) in f32
    // Sensors come in file order (ParseSensorRules below).  SetSensors hands records over directly; an empty vector forgets
    // them; a file, when one is named, goes before them.  With sensors active every launch of ComputeDosageMap and
    // ComputeSegments -- photon launches and gather launches, stops and driven segments -- gathers them after its own tracing
    // and gathers and before its capture or accumulate: uvrt_set_gather_sampling(gatherSampling), uvrt_gather_sensors with
    // the launch's lamp, samples = sensorSamples, seed = sensorLaunches++ (a counter of their own since ResetDosageMap) and
    // photons_equiv = the launch's photons; with reflectance > 0 uvrt_gather_sensors_indirect(reflectance, samples =
    // reflectSamples, seed = the launch's gather seed ^ 0x85EBCA6B) with emitter 0 -- the source plane is the snapshot of the
    // direct plane the launch's bounce has taken -- or, under reflectSided, emitter 1 with use_map = there is a reflectance
    // map; then uvrt_accumulate_sensors(duration).  So a sensor sees the lamp and ONE diffuse bounce in both bounce models:
    // bounces 2..K of reflectBounces do not reach sensors, and neither does a mirror panel's light.  The sensors are uploaded
    // when uvrt_sensor_info says the context has none (a new context) or they are not the ones uploaded last; an upload
    // zeroes their maps.  ResetDosageMap zeroes the maps and the counter.  A plan (PlanDurations) runs no sensor call and
    // leaves the sensor maps alone.  Fatal with sensors active: shardWorld > 1, ComputeIterationsBatched, a group,
    // reduceOverComm, and active mirror panels -- the sensors would not see the panels' light, and silently understating a
    // dosimeter is worse than refusing.  No sensors: every path bit for bit and call for call as before.  Saved as
    // <sensor_map>FILE</sensor_map> and <sensor_samples>S</sensor_samples> after <mirror_map> when a file is named; a name that
    // holds <, > or & cannot stand in a route file and is fatal there.
    std::string sensorMap;
    int sensorSamples = 64;
    std::vector<uvrt_sensor> sensorList;            // the caller's sensors (SetSensors); never the file's
    void SetSensors(const std::vector<uvrt_sensor>& sensors);
    bool HasSensors() const { return !sensorMap.empty() || !sensorList.empty(); }
    // Reads sensorMap's file unless that is what the cache holds; nothing to do without a file name.  Returns an empty string
    // or ParseSensorRules' message.
    std::string PrepareSensorMap();
    // the sensors a launch would gather now: the file's when a file is named (empty until it has been read), else the caller's
    const std::vector<uvrt_sensor>& ActiveSensors() const;
    // The rules file above into *out.  Host only.  Returns an empty string, or what is wrong as "FILE:LINE: reason": an unknown
    // keyword or kind, a wrong count of words, a word that is no finite number, a planar sensor's zero normal, a lattice count
    // that is no integer >= 1, more than 2^24 sensors (or "FILE: cannot be read").
    static std::string ParseSensorRules(const char* path, std::vector<uvrt_sensor>* out);
    // What the sensors have received, one entry per sensor: dose and peak through uvrt_sensor_dosage with exactly the divisor
    // and the scaled power Shade hands to uvrt_shade for the dosage view (mJ/cm^2) and the maxpower view (microW/cm^2);
    // stdErr = scaled_power * sqrt(var_map) / N with the dosage view's two values, in f64 on the host: one standard error of
    // dose, from the direct part's shadow rays alone.
    void ReadSensors(std::vector<float>& dose, std::vector<float>& peak, std::vector<double>& stdErr);
    // Calibration in the room as it stands: the sensor maps are reset, one stop launch at lightPositions[lightIndex] runs for
    // the sensors alone (photonCount photons_equiv, sensorSamples samples, the current reflect options; with reflectance > 0
    // the direct gather and the snapshot or the face planes the bounce needs are made first, in gather mode only), sensor
    // `sensor`'s uvrt_sensor_dosage(UVRT_MAP_MAX, photonCount, 1.0f) is read, calibratedPower = 0.01f * (measurePower / value)
    // and lightIntensity = calibratedPower as CalibratePower sets them, and the sensor maps are reset again.  Fatal when the
    // value is not > 0.  Touches neither the scene nor the triangle maps.
    void CalibratePowerAtSensor(float measurePower, int sensor, int lightIndex);
    unsigned sensorLaunches = 0;                    // sensor launches since ResetDosageMap: the next launch's seed
    static bool InstallSensorHooks();               // (raytracer_sensors.cpp calls it when it is loaded)
    // The batched direct gather (include/uvrt.h "batched direct gather").  gatherBatch = B in [2, 64] with
    // gatherSamples > 0: ComputeDosageMap and ComputeSegments walk their launches in groups of up to B consecutive ones; a
    // group's shadow rays are traced in one uvrt_gather_direct_batch (the seeds the launches would have taken, the variance
    // state on around it when gatherRelError asks for it), and every launch then runs as before with
    // uvrt_gather_batch_select(k) where uvrt_gather_direct stood -- refine, bounce, capture and accumulate after it, the
    // seed counter advancing the same.  B changes no bit of any result, so it is not saved in route files.  Before the first
    // group the ray capacity is raised to min(B, launches) x triangles x gatherSamples rays, 2^23 at most (ClearBuffers puts
    // photonCount back).  0 (default) and 1: launch by launch.  Outside [0, 64]: fatal.
    int gatherBatch = 0;
    unsigned gatherLaunches = 0;                  // gather launches since ResetDosageMap: the next launch's seed
private:
    std::vector<RouteLaunch> Launches() const;      // RouteLaunches of this instance's route
    // How a launch gathers: the knobs above as one value, so that a launch of ComputeDosageMap and a launch of a plan go
    // through the same code.  samples = 0: photons, and nothing else is read.  relError / maxExtra: the refine; reflectance,
    // reflectSamples, reflectBounces, sided, mapped: the bounces; mirrored: the mirror gather; batch: the gather batch;
    // sensors: the virtual dosimeters.
    // Made by OwnGather (the members; mapped and mirrored: there is a map, there are panels) or PlanGather (a plan's own).
    struct GatherOptions {
        int samples = 0, sampling = 0;
        double relError = 0.0;
        int maxExtra = 64;
        float reflectance = 0.0f;
        int reflectSamples = 16, reflectBounces = 0, sided = 0;
        bool mapped = false, mirrored = false;
        int batch = 0;
        bool sensors = false;                       // the launch gathers the sensors too; never set for a plan
    };
    GatherOptions OwnGather() const;
    static GatherOptions PlanGather(const PlanOptions& opt);
    // Why a launch with these options is refused, or null: every condition that ComputeDosageMap's launches and
    // PlanDurations both check, written once.  plan: PlanDurations' wording (it prints it behind "PlanDurations: ").
    // checks: kBatchRefusals are those of a whole list (RunLaunches, on entry), kLaunchRefusals those of every launch.
    enum { kBatchRefusals = 1, kLaunchRefusals = 2 };
    static const char* GatherRefusal(const GatherOptions& g, int checks, bool plan);
    // One launch, as ComputeDosageMap runs it: generate[_sweep] -> extend -> accumulate, or with g.samples > 0 the direct
    // gather -> accumulate_expected, its plane first captured into column captureColumn of a plan when that is >= 0.
    // A stop counts in launchIndex (the shard test) and photonMapSize, a sweep in neither.
    // batchSlot >= 0: the launch's planes are those of launch batchSlot of the context's gather batch (RunLaunches).
    void RunLaunch(const RouteLaunch& launch, int photons, int triangleCount, const GatherOptions& g, int captureColumn, int batchSlot);
    // A list of launches through RunLaunch, in order (capture: every plane into its launch's column of a plan); with
    // g.samples > 0 and g.batch >= 2 in groups of up to g.batch behind one uvrt_gather_direct_batch each (gatherBatch).
    void RunLaunches(const std::vector<RouteLaunch>& list, int photons, int triangleCount, const GatherOptions& g, bool capture);
    // the active map (the file's, read with `base` as every entry's start, or the caller's) into the context's planes when the
    // context has none or the map is not the one uploaded last (RunLaunch)
    void UploadReflectanceMap(int triangleCount, float base);
    // the active panels (the file's or the caller's) into the context when it has none or they are not the ones uploaded last
    void UploadMirrors(int triangleCount);
    // the active sensors into the context when it has none or they are not the ones uploaded last (an upload zeroes their maps)
    void UploadSensors();
    // the sensors' part of a launch: direct gather, one bounce under the launch's reflect options, accumulate (RunLaunch)
    void GatherSensors(const RouteLaunch& launch, int photons, const GatherOptions& g, unsigned gatherSeed, bool accumulate);
    void CheckSensorsAlone(const char* who) const;  // fatal where sensors cannot follow: sharding, a communicator, mirror panels
    void ResetSensors();                            // upload, zero the sensors' maps and their launch counter (ResetDosageMap)
    // How raytracer.cpp reaches raytracer_sensors.cpp, which makes every uvrt_* sensor call of the host layer: set by that file
    // when it is part of the program, so that a program built from raytracer.cpp without it links and runs every path that
    // has no sensors.  Sensors() is fatal without the hooks.
    struct SensorHooks {
        void (RayTracer::*gather)(const RouteLaunch&, int, const GatherOptions&, unsigned, bool);
        void (RayTracer::*reset)();
    };
    static const SensorHooks* sensorHooks;
    static const SensorHooks& Sensors();
    std::string SensorMapPath() const;              // sensorMap as it is opened: a relative name is routeDir's
    std::vector<uvrt_sensor> sensorFileList;        // the cache of sensorMap's file ...
    std::string sensorFileParsed;                   // ... and the path it was read from (empty: nothing cached)
    unsigned long long sensorStampNext = 1, sensorFileStamp = 0, sensorValuesStamp = 0, sensorUploaded = 0;
    std::string MirrorMapPath() const;              // mirrorMap as it is opened: a relative name is routeDir's
    std::vector<uvrt_mirror> mirrorFilePanels;      // the cache of mirrorMap's file ...
    std::vector<uint8_t> mirrorFilePanelOfTri;
    std::string mirrorFileParsed;                   // ... and the path it was read from (empty: nothing cached)
    unsigned long long mirrorStampNext = 1, mirrorFileStamp = 0, mirrorValuesStamp = 0, mirrorUploaded = 0;
    std::string ReflectMapPath() const;             // reflectMap as it is opened: a relative name is routeDir's
    std::vector<float> reflectFileValues;           // the cache of reflectMap's file ...
    std::string reflectFileParsed;                  // ... the path it was read from (empty: nothing cached) ...
    float reflectFileBase = 0.0f;                   // ... and the base it was read with
    // every change of either source takes a new stamp; the context's planes hold the source with stamp reflectUploaded (0: none)
    unsigned long long reflectStampNext = 1, reflectFileStamp = 0, reflectValuesStamp = 0, reflectUploaded = 0;
    long long rayCapacity = 0;                      // what ClearBuffers / RunLaunches last gave uvrt_resize_rays
    struct ShadeArguments { int which_map, photons_per_light; float scaled_power, min_value; };
    ShadeArguments ShadeArgs() const;               // what Shade passes on for viewMode (raytracer.cpp:96-116)
    static void TraceBatched(const std::vector<RayTracer*>& group, int iterations);
    // the steps of PlanDurations: capture (photon counts or the direct gather), then bounds and solve
    static void PlanCaptureCounts(const std::vector<RayTracer*>& group, int cols);
    void PlanCaptureGather(const std::vector<RouteLaunch>& list, const GatherOptions& g, double confidence);
    static std::vector<float> PlanSolve(const std::vector<RayTracer*>& group, const PlanOptions& opt, const std::vector<RouteLaunch>& list,
                                        uvrt_plan_report* rep, uvrt_plan_bounds_report* brep);
public:
    // The reference never reads the dose back; the headless build does.
    void ReadDosage(float* out, int first, int count);
    void Sync();                        // clFinish(Kernel::GetQueue()), myapp.cpp:165
};

}  // namespace Tmpl8

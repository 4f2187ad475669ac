// raytracer_internal.h -- what the translation units of the host layer share and nobody else sees: the fatal-error idiom,
// a rules file's number, the uvrt_gather_params of a launch.  raytracer.cpp is the orchestration; raytracer_sensors.cpp holds
// the virtual dosimeters (raytracer.h sensorMap), which it reaches through RayTracer::sensorHooks alone.
#pragma once
#include "raytracer.h"

#include <cmath>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>

namespace Tmpl8 {
namespace host_internal {

// template.cpp:904-917 FatalError: report and terminate
inline void check(int rc, const char* what)
{
    if (rc == UVRT_OK) return;
    fprintf(stderr, "Fatal error in %s: %s\n", what, uvrt_last_error());
    exit(1);
}
inline void fatal(const char* what)
{
    fprintf(stderr, "Fatal error: %s\n", what);
    exit(1);
}

// a whole word as a number: a double, rounded once to f32
inline bool rule_number(const std::string& w, float* out)
{
    if (w.empty()) return false;
    char* end = nullptr;
    const double v = strtod(w.c_str(), &end);
    if (end != w.c_str() + w.size() || std::isnan(v)) return false;
    *out = (float)v;
    return true;
}

// the uvrt_gather_params of a gather launch with seed `seed`
inline uvrt_gather_params gather_params(const RouteLaunch& l, float lightLength, int samples, unsigned seed, int photons)
{
    uvrt_gather_params g;
    memset(&g, 0, sizeof g);
    memcpy(g.from, l.from, 12);
    memcpy(g.to, l.kind == UVRT_LAUNCH_SWEEP ? l.to : l.from, 12);       // from == to: a stop
    g.light_length = lightLength;
    g.samples = samples;
    g.seed = seed;
    g.photons_equiv = photons;
    return g;
}

}  // namespace host_internal
}  // namespace Tmpl8

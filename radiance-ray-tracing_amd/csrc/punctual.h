// punctual.h -- launch declarations of rdx_punctual_light_hits and rdx_trace_paths_punctual (punctual.hip): the direct term of one
// record of a caller's light table -- directional, point or spot -- on material records, and the shade kernel of a bounce that
// samples every record of the table at every hit.  The streams of a bounce and its fold kernel are those of
// rdx_trace_paths_lights (light_paths.h: LightPathStreams, launch_lights_fold), unchanged; the scene view and the bounds rule are
// those of rdx_shade_hits (shade.h: ShadeScene, shade_in_bounds), unchanged.
#pragma once
#include <stdint.h>

#include "light_paths.h"
#include "rdx_types.h"
#include "shade.h"

namespace rdx {

#if defined(__HIPCC__)
// rdx_punctual_light_hits: n rays (only the direction is read) and their material records in; the direct term of the one table
// record `light` out (rgb, 0) and -- optional -- the shadow ray towards it, whose tmax is the distance to a point or spot light.
// A record that is dark at a hit writes zeros to both.  Gathers nothing: no record can make it read outside a buffer.
void launch_punctual_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const PunctualLight* light, float4* lit,
                                float4* shadow);
// k_punctual_shade: launch_lights_shade (light_paths.h) with records 0 .. nLights - 1 of the table `lights` in the place of the
// scene's DirLights; counters, compaction and every stream as there.
void launch_punctual_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                           uint32_t nLights, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext, uint32_t* live,
                           uint32_t* invalid);
#endif

} // namespace rdx

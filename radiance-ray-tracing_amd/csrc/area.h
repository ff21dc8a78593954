// area.h -- the record and the launch declarations of rdx_area_light_hits and rdx_trace_paths_area (area.hip): the direct term of
// one record of a caller's AREA light table -- a parallelogram or a triangle of constant radiance, sampled at one point per (hit,
// light) -- on material records, and the shade kernel of a bounce that samples every record of a punctual table and then every
// record of an area table at every hit.  The streams of a bounce and its fold kernel are those of rdx_trace_paths_lights
// (light_paths.h: LightPathStreams, launch_lights_fold), unchanged; the scene view and the bounds rule are those of rdx_shade_hits
// (shade.h: ShadeScene, shade_in_bounds), unchanged; the punctual record is rdx_types.h' PunctualLight, unchanged.  The area record
// lives here, not in rdx_types.h, so that no header an existing device unit includes changes.
#pragma once
#include <stdint.h>

#include "light_paths.h"
#include "rdx_types.h"
#include "shade.h"

namespace rdx {

// a record of a caller's area light table (include/rdx.h rdx_area_light; no reference counterpart): four float4
enum : uint32_t { AREA_QUAD = 0u, AREA_TRIANGLE = 1u, AREA_TWO_SIDED = 1u };
struct AreaLight { float corner[3]; uint32_t type; float edgeU[3]; uint32_t flags; float edgeV[3]; float _0; float radiance[3]; float _1; };
static_assert(sizeof(AreaLight) == 64, "area light table record");

#if defined(__HIPCC__)
// rdx_area_light_hits: n rays (only the direction is read), their material records and one key or one float4 of randoms per ray in
// (exactly one of `keys` and `randoms` is given; `stream` is read on the keys route alone); the direct term of the one table record
// `light` out (rgb, 0) and -- optional -- the shadow ray towards the sampled point, which stops short of it.  A record that is dark
// at a hit writes zeros to both.  Gathers nothing: no record can make it read outside a buffer.
void launch_area_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const AreaLight* light, const uint4* keys,
                            uint32_t stream, const float4* randoms, float4* lit, float4* shadow);
// k_area_shade: launch_punctual_shade (punctual.h) with records 0 .. nArea - 1 of the table `area` after the nLights punctual
// records: nLights + nArea records per survivor, punctual records first; counters, compaction and every stream as there.
void launch_area_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                       uint32_t nLights, const AreaLight* area, uint32_t nArea, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext,
                       uint32_t* live, uint32_t* invalid);
#endif

} // namespace rdx

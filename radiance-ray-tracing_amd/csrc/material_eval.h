// material_eval.h -- launch declarations of rdx_resolve_materials and rdx_light_hits (material.hip): the evaluated material of a
// query's hits, and one directional light's direct term on such records.  The scene view and the bounds rule are those of
// rdx_shade_hits (shade.h: ShadeScene, shade_in_bounds), unchanged.
#pragma once
#include <stdint.h>

#include "rdx_types.h"
#include "shade.h"

namespace rdx {

#if defined(__HIPCC__)
// rdx_resolve_materials: n rays and their closest-hit query records in; one 64-byte material record per ray out (four float4: N |
// hit, albedo | materialIndex, metallic roughness transmission ior, above | 0), zeros for everything that is not a valid hit.
// *invalid += records that fail shade_in_bounds.  All pointers are device pointers.
void launch_resolve_materials(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits,
                              uint32_t n, const ShadeScene& sc, float4* out, uint32_t* invalid);
// rdx_light_hits: n rays (only the direction is read) and their material records in; the direct term of the one DirLight `light`
// out (rgb, 0) and -- optional -- the shadow ray towards it.  Gathers nothing: no record can make it read outside a buffer.
void launch_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const DirLight* light, float4* lit, float4* shadow);
#endif

} // namespace rdx

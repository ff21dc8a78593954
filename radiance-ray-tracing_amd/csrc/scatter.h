// scatter.h -- launch declaration of rdx_scatter_hits (scatter.hip): the next-direction sample of the stock closest-hit shader
// `material` on material records -- the half of the shader that rdx_resolve_materials and rdx_light_hits (material_eval.h) leave.
#pragma once
#include <stdint.h>

#include "rdx_types.h"

namespace rdx {

#if defined(__HIPCC__)
// rdx_scatter_hits: n rays (only the direction is read), their material records, their surface records (only `below` is read) and
// one key (pcg3d's three inputs) or one float4 of randoms (xyz used as they are) per ray in -- exactly one of `keys` / `randoms`
// is given; one 16-byte scatter record per ray out (nextFactor | slot), and the next ray of every survivor.  `src` given: the
// survivors are packed by *live, the compaction cursor (k_shade_hits' rule); *live counts them either way and must be zero
// before the launch.  Gathers nothing: no record can make it read outside a buffer.  All pointers are device pointers.
void launch_scatter_hits(hipStream_t st, const float4* rays, const float4* materials, const float4* surfaces, const uint4* keys,
                         const float4* randoms, uint32_t n, float4* scatter, float4* next, uint32_t* src, uint32_t* live);
#endif

} // namespace rdx

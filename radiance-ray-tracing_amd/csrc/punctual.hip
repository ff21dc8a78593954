// punctual.hip -- device side of rdx_punctual_light_hits and rdx_trace_paths_punctual: the direct term of one record of a caller's
// light table -- directional, point or spot (include/rdx.h rdx_punctual_light) -- on material records, and the shade kernel of a
// bounce that samples every record of the table at every hit:
//
//   closest-hit query -> k_punctual_shade -> any-hit query of live x L shadow rays -> k_lights_fold (light_paths.hip)
//
// Both kernels are callers of shared text: what a record emits at a hit is punctual_emit and the record it leaves is light_record
// (light_emit.h), for the per-hit kernel and the shade kernel alike, so the per-path call has the bits of the per-hit call; the
// shade kernel is path_shade.h's body over the table.  A translation unit of its own, so that the code objects of kernels.hip,
// surface.hip, shade.hip, scatter.hip, paths.hip, raygen.hip and tlas_update.hip stay the ones they were, bit for bit
// (profiles/punctual_kernels.txt).
#include "kernels.h"

#include "path_shade.h"
#include "punctual.h"

namespace rdx {

// light_hits (light_emit.h) with one record of the table.
__global__ void __launch_bounds__(LIGHT_HITS_BLOCK)
k_punctual_light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, const PunctualLight* __restrict__ light,
                      float4* __restrict__ lit, float4* __restrict__ shadow)
{
    light_hits(rays, mats, n, lit, shadow,
               [=](uint32_t, const f3& above, f3& L, f3& E, float& tmax) { return punctual_emit(light, above, L, E, tmax); });
}

// path_shade over records 0 .. nLights - 1 of the table: k_punctual_light_hits for record j.
__global__ void __launch_bounds__(PATH_SHADE_BLOCK)
k_punctual_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc,
                 const PunctualLight* __restrict__ lights, uint32_t nLights, LightPathStreams io, uint32_t n, uint32_t depth, uint32_t sampleNext,
                 uint32_t* __restrict__ live, uint32_t* __restrict__ invalid)
{
    path_shade(insts, slotOf, nInst, sc, PunctualSource{lights, nLights}, io, n, depth, sampleNext, live, invalid);
}

void launch_punctual_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const PunctualLight* light, float4* lit,
                                float4* shadow)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LIGHT_HITS_BLOCK - 1) / LIGHT_HITS_BLOCK);
    hipLaunchKernelGGL(k_punctual_light_hits, dim3(blocks), dim3(LIGHT_HITS_BLOCK), 0, st, rays, materials, n, light, lit, shadow);
}

void launch_punctual_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                           uint32_t nLights, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext, uint32_t* live,
                           uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PATH_SHADE_BLOCK - 1) / PATH_SHADE_BLOCK);
    hipLaunchKernelGGL(k_punctual_shade, dim3(blocks), dim3(PATH_SHADE_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, io, n, depth,
                       sampleNext ? 1u : 0u, live, invalid);
}

} // namespace rdx

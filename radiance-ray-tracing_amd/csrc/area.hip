// area.hip -- device side of rdx_area_light_hits and rdx_trace_paths_area: the direct term of one record of a caller's area light
// table -- a parallelogram or a triangle of constant radiance (include/rdx.h rdx_area_light), sampled at ONE point per (hit, light)
// -- on material records, and the shade kernel of a bounce that samples every record of a punctual table and then every record of
// an area table at every hit:
//
//   closest-hit query -> k_area_shade -> any-hit query of live x (L + A) shadow rays -> k_lights_fold (light_paths.hip)
//
// Both kernels are callers of shared text: what an area record emits at a hit is area_emit and the record it leaves is
// light_record (light_emit.h), for the per-hit kernel and the shade kernel alike, so the per-path call has the bits of the per-hit
// call; the shade kernel is path_shade.h's body over the two tables, its punctual half the very function of k_punctual_shade
// (punctual.hip).  A translation unit of its own, so that the code objects of kernels.hip, surface.hip, shade.hip, scatter.hip,
// paths.hip, raygen.hip and tlas_update.hip stay the ones they were, bit for bit (profiles/area_kernels.txt).
#include "kernels.h"

#include "area.h"
#include "path_shade.h"

namespace rdx {

// light_hits (light_emit.h) with one record of the area table and key i = keys[i] or randoms i = randoms[i] (exactly one of the two
// pointers is given).  The random pair of the keys route is area_random(frameID, pixel, depth, stream).xy.
__global__ void __launch_bounds__(LIGHT_HITS_BLOCK)
k_area_light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, const AreaLight* __restrict__ light,
                  const uint4* __restrict__ keys, uint32_t stream, const float4* __restrict__ randoms, float4* __restrict__ lit,
                  float4* __restrict__ shadow)
{
    light_hits(rays, mats, n, lit, shadow, [=](uint32_t i, const f3& above, f3& L, f3& E, float& tmax) {
        float u, v;
        if (keys) {
            const uint4 key = keys[i];
            const f3 rnd = area_random(key.x, key.y, key.z, stream);
            u = rnd.x; v = rnd.y;
        } else {
            const float4 r = randoms[i];
            u = r.x; v = r.y;
        }
        return area_emit(light, above, u, v, L, E, tmax);
    });
}

// path_shade over records 0 .. nLights - 1 of the punctual table, then records 0 .. nArea - 1 of the area table: nLights + nArea
// records per survivor.
__global__ void __launch_bounds__(PATH_SHADE_BLOCK)
k_area_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc,
             const PunctualLight* __restrict__ lights, uint32_t nLights, const AreaLight* __restrict__ area, uint32_t nArea, LightPathStreams io,
             uint32_t n, uint32_t depth, uint32_t sampleNext, uint32_t* __restrict__ live, uint32_t* __restrict__ invalid)
{
    path_shade(insts, slotOf, nInst, sc, PunctualAreaSource{lights, nLights, area, nArea}, io, n, depth, sampleNext, live, invalid);
}

void launch_area_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const AreaLight* light, const uint4* keys,
                            uint32_t stream, const float4* randoms, float4* lit, float4* shadow)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LIGHT_HITS_BLOCK - 1) / LIGHT_HITS_BLOCK);
    hipLaunchKernelGGL(k_area_light_hits, dim3(blocks), dim3(LIGHT_HITS_BLOCK), 0, st, rays, materials, n, light, keys, stream, randoms, lit, shadow);
}

void launch_area_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                       uint32_t nLights, const AreaLight* area, uint32_t nArea, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext,
                       uint32_t* live, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PATH_SHADE_BLOCK - 1) / PATH_SHADE_BLOCK);
    hipLaunchKernelGGL(k_area_shade, dim3(blocks), dim3(PATH_SHADE_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, area, nArea, io, n, depth,
                       sampleNext ? 1u : 0u, live, invalid);
}

} // namespace rdx

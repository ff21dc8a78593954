// light_paths.hip -- device side of rdx_trace_paths_lights: one bounce of a path tracer that samples EVERY directional light of the
// scene at every hit, fused into two kernels around the any-hit query of the bounce's shadow rays (include/rdx.h).
//
//   closest-hit query -> k_lights_shade -> any-hit query of live x L shadow rays -> k_lights_fold
//
// k_lights_shade is path_shade.h's body over the scene buffer's DirLight array; k_punctual_shade (punctual.hip) and k_area_shade
// (area.hip) are the same body over a caller's tables, and all three hand over to k_lights_fold below.  A translation unit of its
// own, so that the code objects of kernels.hip, surface.hip, shade.hip, scatter.hip, paths.hip, raygen.hip and tlas_update.hip stay
// the ones they were, bit for bit (profiles/light_paths_kernels.txt).
#include "kernels.h"

#include "light_paths.h"
#include "path_shade.h"

namespace rdx {

constexpr uint32_t LIGHT_PATHS_BLOCK = 256;

// path_shade over the scene's first nLights DirLights: k_light_hits (material.hip) for light j = 0 .. L - 1.
__global__ void __launch_bounds__(PATH_SHADE_BLOCK)
k_lights_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc, const DirLight* __restrict__ lights,
               uint32_t nLights, LightPathStreams io, uint32_t n, uint32_t depth, uint32_t sampleNext, uint32_t* __restrict__ live,
               uint32_t* __restrict__ invalid)
{
    path_shade(insts, slotOf, nInst, sc, DirLightSource{lights, nLights}, io, n, depth, sampleNext, live, invalid);
}

// One survivor per lane.  A path has at most one live ray, so radiance[path] and the weight are plain loads and stores: no atomics,
// no LDS.  Every float32 operation is rounded on its own (this unit is compiled with -ffp-contract=off), in the order of the
// README's loop: direct = ((0 + x_0) + x_1) + ..., x_j = occluded ? 0 : lit_j; radiance = direct + ambient; color += weight *
// radiance; weight *= nextFactor.
__global__ void __launch_bounds__(LIGHT_PATHS_BLOCK)
k_lights_fold(const float4* __restrict__ any, uint32_t nLights, LightPathStreams io, uint32_t n)
{
    const uint32_t k = blockIdx.x * LIGHT_PATHS_BLOCK + threadIdx.x;
    if (k >= n) return;
    f3 direct = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (uint32_t j = 0; j < nLights; ++j) {
        const size_t r = (size_t)k * nLights + j;
        const bool occluded = __float_as_uint(any[2 * r].w) == 1u;
        const float4 l = io.lit[r];
        direct = direct + (occluded ? mk3(0.0f, 0.0f, 0.0f) : mk3(l.x, l.y, l.z));
    }
    const float4 a = io.foldA[k], f = io.foldF[k], w = io.nWeight[k];
    const uint32_t path = io.nIds[k].x;
    const f3 radiance = direct + mk3(a.x, a.y, a.z);
    const float4 c = io.radiance[path];
    const f3 weight = mk3(w.x, w.y, w.z);
    const f3 color = mk3(c.x, c.y, c.z) + weight * radiance;
    const f3 next = weight * mk3(f.x, f.y, f.z);
    io.radiance[path] = make_float4(color.x, color.y, color.z, 0.0f);
    io.nWeight[k] = make_float4(next.x, next.y, next.z, 0.0f);
}

void launch_lights_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const DirLight* lights,
                         uint32_t nLights, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext, uint32_t* live,
                         uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PATH_SHADE_BLOCK - 1) / PATH_SHADE_BLOCK);
    hipLaunchKernelGGL(k_lights_shade, dim3(blocks), dim3(PATH_SHADE_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, io, n, depth,
                       sampleNext ? 1u : 0u, live, invalid);
}

void launch_lights_fold(hipStream_t st, const float4* any, uint32_t nLights, const LightPathStreams& io, uint32_t live)
{
    if (!live) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)live + LIGHT_PATHS_BLOCK - 1) / LIGHT_PATHS_BLOCK);
    hipLaunchKernelGGL(k_lights_fold, dim3(blocks), dim3(LIGHT_PATHS_BLOCK), 0, st, any, nLights, io, live);
}

} // namespace rdx

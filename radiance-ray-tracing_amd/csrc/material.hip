// material.hip -- device side of rdx_resolve_materials and rdx_light_hits: what the stock closest-hit shader `material` (stages.h)
// evaluates before its light term, as a record per hit, and that light term for any one of the scene's directional lights
// (include/rdx.h rdx_material_record).
//
// Both kernels are callers of shared text: the fenced gather and the evaluation are hit_material.h's, which the shade kernels of
// the path calls use as well (path_shade.h); the light term is light_emit.h's, shared with rdx_punctual_light_hits,
// rdx_area_light_hits and those shade kernels.  A translation unit of its own, so that the code objects of kernels.hip,
// surface.hip, shade.hip and paths.hip stay the ones they were, bit for bit (profiles/material_kernels.txt).
#include "kernels.h"

#include "hit_material.h"
#include "light_emit.h"
#include "material_eval.h"

namespace rdx {

constexpr uint32_t MATERIAL_BLOCK = 256;

// One ray per thread: ray i = rays[2i], rays[2i + 1], record i = hits[2i], hits[2i + 1] (as k_shade_hits), material record i =
// out[4i .. 4i + 3]: adjacent lanes read adjacent 32-byte records and write adjacent 64-byte ones.  A record that fails gather_hit
// writes zeros and is counted -- one ballot per wave, one atomic by its first lane, and only where the wave has such a record.
__global__ void __launch_bounds__(MATERIAL_BLOCK)
k_resolve_materials(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, const float4* __restrict__ rays,
                    const float4* __restrict__ hits, uint32_t n, ShadeScene sc, float4* __restrict__ out, uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * MATERIAL_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float4 ro = rays[2 * (size_t)i], rd = rays[2 * (size_t)i + 1];
        const float4 ha = hits[2 * (size_t)i], hb = hits[2 * (size_t)i + 1];
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
        if (__float_as_uint(ha.w) == 1u) {
            HitGather g;
            if (gather_hit(sc, slotOf, nInst, hb, g)) {
                HitMaterial m;
                eval_hit_material(sc, insts, ro, rd, ha, g, m);
                r0 = make_float4(m.N.x, m.N.y, m.N.z, __uint_as_float(1u));
                r1 = make_float4(m.albedo.x, m.albedo.y, m.albedo.z, __uint_as_float((uint32_t)m.materialIndex));
                r2 = make_float4(m.metallic, m.roughness, m.transmission, m.ior);
                r3 = make_float4(m.above.x, m.above.y, m.above.z, 0.0f);        // the shadow ray's origin
            } else {
                bad = true;
            }
        }
        float4* o = out + 4 * (size_t)i;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    }
    // wave64 ballot: every lane of the wave is here (no thread has returned)
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (uint32_t)__popcll(m));
}

// light_hits (light_emit.h) with one DirLight of the scene buffer: the same address in every lane, so its eight floats arrive
// through the scalar cache.
__global__ void __launch_bounds__(LIGHT_HITS_BLOCK)
k_light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, const DirLight* __restrict__ light,
             float4* __restrict__ lit, float4* __restrict__ shadow)
{
    light_hits(rays, mats, n, lit, shadow, [=](uint32_t, const f3&, f3& L, f3& E, float& tmax) { return dir_emit(light, L, E, tmax); });
}

void launch_resolve_materials(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits,
                              uint32_t n, const ShadeScene& sc, float4* out, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + MATERIAL_BLOCK - 1) / MATERIAL_BLOCK);
    hipLaunchKernelGGL(k_resolve_materials, dim3(blocks), dim3(MATERIAL_BLOCK), 0, st, insts, slotOf, nInst, rays, hits, n, sc, out, invalid);
}

void launch_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const DirLight* light, float4* lit, float4* shadow)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LIGHT_HITS_BLOCK - 1) / LIGHT_HITS_BLOCK);
    hipLaunchKernelGGL(k_light_hits, dim3(blocks), dim3(LIGHT_HITS_BLOCK), 0, st, rays, materials, n, light, lit, shadow);
}

} // namespace rdx

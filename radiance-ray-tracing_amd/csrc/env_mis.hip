// env_mis.hip -- device side of rdx_env_mis_weights and rdx_trace_paths_env_mis (include/rdx.h): the environment and
// the scatter sample weighted against each other by the balance heuristic, so that a bounce ray that leaves the scene is seen --
//
//   k_env_mis_weights  one direction per lane: the weight, the two densities and the lobe (env_mis.h) for a `shadow` or `next` row
//   k_env_mis_shade    path_shade.h's body over the punctual table, the area table and the environment, with EnvMis
//   k_env_mis_fold     k_lights_fold with the weight's fourth word handed on
//
// -- all three around the ONE text of env_mis.h, so the per-path call has the bits of the loop over the per-hit calls.  A
// translation unit of its own, so that the code objects of the other units stay the ones they were (profiles/env_mis_kernels.txt).
#include "kernels.h"

#include "env.h"
#include "env_mis.h"
#include "path_shade.h"

namespace rdx {

constexpr uint32_t ENV_MIS_BLOCK = 256;

// Direction k = dirs[2k + 1] belongs to ray / material record s = src ? src[k] : k -- the one gather, held to nrecords.  A record
// whose `hit` is not 1, an s outside the records and a row that accepts nothing (tmax 0: a dark `shadow` row, a dead `next` row) or
// has no direction give 16 zero bytes.  The lobe is that of the random triple rdx_scatter_hits was given for record s; without
// keys and randoms the direction is the environment's own (NONE).  No LDS, no atomics; the table's header comes through the scalar
// cache as in env_emit.
__global__ void __launch_bounds__(ENV_MIS_BLOCK)
k_env_mis_weights(const float4* __restrict__ rays, const float4* __restrict__ mats, const float4* __restrict__ dirs, uint32_t n,
                  const uint32_t* __restrict__ src, uint32_t nrecords, const uint4* __restrict__ keys, const float4* __restrict__ randoms, EnvView env,
                  uint4* __restrict__ out)
{
    const uint32_t k = blockIdx.x * ENV_MIS_BLOCK + threadIdx.x;
    if (k >= n) return;
    uint4 o = make_uint4(0u, 0u, 0u, 0u);
    const uint32_t s = src ? src[k] : k;
    const float4 d = dirs[2 * (size_t)k + 1];
    if (s < nrecords && d.w != 0.0f && !(d.x == 0.0f && d.y == 0.0f && d.z == 0.0f)) {
        const float4 rd = rays[2 * (size_t)s + 1];
        const float4 m0 = mats[4 * (size_t)s], m2 = mats[4 * (size_t)s + 2];
        if (__float_as_uint(m0.w) == 1u) {
            uint32_t lobe = LOBE_NONE;
            if (keys) {
                const uint4 key = keys[s];
                lobe = lobe_of(pcg3d(key.x, key.y, key.z), m2.z);
            } else if (randoms) {
                const float4 r = randoms[s];
                lobe = lobe_of(mk3(r.x, r.y, r.z), m2.z);
            }
            const f3 V = normalize3(-mk3(rd.x, rd.y, rd.z));
            const MisWeight w = env_mis_weight(env, mk3(m0.x, m0.y, m0.z), V, mk3(d.x, d.y, d.z), m2.y, m2.z, lobe);
            o = make_uint4(__float_as_uint(w.w), __float_as_uint(w.pScatter), __float_as_uint(w.pEnv), lobe);
        }
    }
    out[k] = o;
}

// what path_shade adds for this call: the weights of env_mis.h at the shaded point
struct EnvMis {
    static constexpr bool on = true;
    EnvView env;
    __device__ __forceinline__ float skyWeight(const ShadePoint& p, const f3& L) const
    {
        return env_mis_weight(env, p.N, p.V, L, p.roughness, p.transmission, LOBE_NONE).w;
    }
    __device__ __forceinline__ float scatterWeight(const ShadePoint& p, const f3& L, const f3& rnd) const
    {
        return env_mis_weight(env, p.N, p.V, L, p.roughness, p.transmission, lobe_of(rnd, p.transmission)).w;
    }
};

__global__ void __launch_bounds__(PATH_SHADE_BLOCK)
k_env_mis_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc,
                const PunctualLight* __restrict__ lights, uint32_t nLights, const AreaLight* __restrict__ area, uint32_t nArea, EnvView env,
                LightPathStreams io, uint32_t n, uint32_t depth, uint32_t sampleNext, uint32_t* __restrict__ live, uint32_t* __restrict__ invalid)
{
    path_shade(insts, slotOf, nInst, sc, PunctualAreaEnvSource{lights, nLights, area, nArea, env}, io, n, depth, sampleNext, live, invalid, EnvMis{env});
}

// k_lights_fold (light_paths.hip), statement for statement, with ONE difference: foldF.w -- w_scatter of the direction the shade
// kernel sampled -- is handed on in nWeight.w, where the next depth's shade finds it with the path's weight.  A fold of this unit's
// own and not a template both units call: that moves k_lights_fold's code (profiles/env_mis_kernels.txt).
__global__ void __launch_bounds__(ENV_MIS_BLOCK)
k_env_mis_fold(const float4* __restrict__ any, uint32_t nLights, LightPathStreams io, uint32_t n)
{
    const uint32_t k = blockIdx.x * ENV_MIS_BLOCK + threadIdx.x;
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
    io.nWeight[k] = make_float4(next.x, next.y, next.z, f.w);
}

void launch_env_mis_weights(hipStream_t st, const float4* rays, const float4* materials, const float4* dirs, uint32_t n, const uint32_t* src,
                            uint32_t nrecords, const uint4* keys, const float4* randoms, const EnvView& env, uint4* out)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + ENV_MIS_BLOCK - 1) / ENV_MIS_BLOCK);
    hipLaunchKernelGGL(k_env_mis_weights, dim3(blocks), dim3(ENV_MIS_BLOCK), 0, st, rays, materials, dirs, n, src, nrecords, keys, randoms, env, out);
}

void launch_env_mis_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                          uint32_t nLights, const AreaLight* area, uint32_t nArea, const EnvView& env, const LightPathStreams& io, uint32_t n,
                          uint32_t depth, bool sampleNext, uint32_t* live, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PATH_SHADE_BLOCK - 1) / PATH_SHADE_BLOCK);
    hipLaunchKernelGGL(k_env_mis_shade, dim3(blocks), dim3(PATH_SHADE_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, area, nArea, env, io, n,
                       depth, sampleNext ? 1u : 0u, live, invalid);
}

void launch_env_mis_fold(hipStream_t st, const float4* any, uint32_t nLights, const LightPathStreams& io, uint32_t live)
{
    if (!live) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)live + ENV_MIS_BLOCK - 1) / ENV_MIS_BLOCK);
    hipLaunchKernelGGL(k_env_mis_fold, dim3(blocks), dim3(ENV_MIS_BLOCK), 0, st, any, nLights, io, live);
}

} // namespace rdx

// scatter.hip -- device side of rdx_scatter_hits: the second half of the stock closest-hit shader `material` (stages.h) -- the
// next-direction sample, nextFactor and the choice between the two offset origins -- on the material records of
// rdx_resolve_materials and the surface records of rdx_resolve_hits (include/rdx.h rdx_scatter).
//
// A translation unit of its own, like surface.hip, shade.hip and material.hip and for the same reason: the code objects of
// kernels.hip, surface.hip, shade.hip, material.hip, paths.hip, raygen.hip and tlas_update.hip stay the ones they were, bit for bit
// (profiles/scatter_kernels.txt).  make_frame, sample_brdf_transm and pcg3d are those of stages.h / device_math.h, called as
// `material` calls them (stages.h:278, 311, 317-324).
//
// The identity with rdx_shade_hits and with the reference's recorded payloads is stated for hits whose SBT row is `material`
// (instanceSBTOffset 0): a record says nothing about the row, and this kernel runs `material`'s sample on every record with
// hit == 1.
#include "kernels.h"

#include "device_math.h"
#include "scatter.h"
#include "stages.h"

namespace rdx {

constexpr uint32_t SCATTER_BLOCK = 256;

// One record per thread: the direction of ray i = rays[2i + 1], material record i = mats[4i .. 4i + 3], `below` of surface record i =
// surfs[4i + 3], key i = keys[i] or randoms i = randoms[i] (exactly one of the two pointers is given); scatter[i] = (nextFactor |
// k).  A surviving ray's next ray goes to record k of `next`: k = i, or -- `src` given -- the wave's base from ONE atomic on *live
// by its first lane plus the ray's rank in the wave's ballot, so the survivors of 64 consecutive inputs stay together and in input
// order (k_shade_hits' rule).  *live counts the survivors either way.  Nothing is gathered, so nothing is fenced; no LDS.
__global__ void __launch_bounds__(SCATTER_BLOCK)
k_scatter_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, const float4* __restrict__ surfs, const uint4* __restrict__ keys,
               const float4* __restrict__ randoms, uint32_t n, float4* __restrict__ scatter, float4* __restrict__ next, uint32_t* __restrict__ src,
               uint32_t* __restrict__ live)
{
    const uint32_t i = blockIdx.x * SCATTER_BLOCK + threadIdx.x;
    const bool active = i < n;
    bool alive = false;
    f3 nf = mk3(0.f, 0.f, 0.f), nd = nf, origin = nf;
    if (active) {
        const float4 rd = rays[2 * (size_t)i + 1];
        const float4 m0 = mats[4 * (size_t)i], m1 = mats[4 * (size_t)i + 1], m2 = mats[4 * (size_t)i + 2], m3 = mats[4 * (size_t)i + 3];
        const float4 s3 = surfs[4 * (size_t)i + 3];
        f3 rnd;
        if (keys) {
            const uint4 key = keys[i];
            rnd = pcg3d(key.x, key.y, key.z);
        } else {
            const float4 r = randoms[i];
            rnd = mk3(r.x, r.y, r.z);
        }
        if (__float_as_uint(m0.w) == 1u) {      // any other value of `hit`: (0, 0, 0 | 0xffffffff), no survivor
            const f3 N = mk3(m0.x, m0.y, m0.z), albedo = mk3(m1.x, m1.y, m1.z);
            const f3 V = normalize3(-mk3(rd.x, rd.y, rd.z));
            NFrame FN;
            make_frame(N, FN);
            nd = sample_brdf_transm(FN, V, N, albedo, m2.x, m2.y, m2.z, m2.w, rnd, nf);
            origin = dot3(nd, N) < 0 ? mk3(s3.x, s3.y, s3.z) : mk3(m3.x, m3.y, m3.z);      // getHitPosition(hitData, -+faceN)
            alive = true;
        }
    }
    // wave64 ballot: every lane of the wave is here (no thread has returned)
    const unsigned long long m = __ballot(alive);
    const uint32_t lane = __lane_id();
    uint32_t base = 0u;
    if (m != 0ull) {
        if (lane == 0u) base = atomicAdd(live, (uint32_t)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    }
    if (!active) return;
    const uint32_t k = src ? base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) : i;
    scatter[i] = make_float4(nf.x, nf.y, nf.z, __uint_as_float(alive ? k : 0xffffffffu));
    if (alive) {
        next[2 * (size_t)k] = make_float4(origin.x, origin.y, origin.z, 0.001f);
        next[2 * (size_t)k + 1] = make_float4(nd.x, nd.y, nd.z, 1000.0f);
        if (src) src[k] = i;
    } else if (!src) {      // not compacting: record i of a ray that does not survive is a ray that accepts nothing (tmax = 0)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        next[2 * (size_t)i] = z; next[2 * (size_t)i + 1] = z;
    }
}

void launch_scatter_hits(hipStream_t st, const float4* rays, const float4* materials, const float4* surfaces, const uint4* keys,
                         const float4* randoms, uint32_t n, float4* scatter, float4* next, uint32_t* src, uint32_t* live)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + SCATTER_BLOCK - 1) / SCATTER_BLOCK);
    hipLaunchKernelGGL(k_scatter_hits, dim3(blocks), dim3(SCATTER_BLOCK), 0, st, rays, materials, surfaces, keys, randoms, n, scatter, next, src, live);
}

} // namespace rdx

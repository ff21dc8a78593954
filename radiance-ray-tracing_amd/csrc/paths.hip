// paths.hip -- device side of rdx_trace_paths: the caller's rays, the records of their first segment and their keys become paths
// of the frame path's streams (kernels.h PathStreams); every stage after that is the frame path's own.
//
// A translation unit of its own, like shade.hip and raygen.hip and for the same reason: the code object of kernels.hip stays the
// one it was, bit for bit (profiles/paths_kernels.txt).
#include "kernels.h"

#include "paths.h"

namespace rdx {

constexpr uint32_t PATHS_INGEST_BLOCK = 256;
constexpr uint32_t PATHS_MISS = 0xffffffffu;         // PathStreams::hitInst of a path whose segment hit nothing (kernels.hip RDX_MISS)

// Five 16-byte loads and five 16-byte stores per lane, adjacent lanes on adjacent records, plus the slot word: no LDS, no atomics.
// The only gather is slotOf[instanceIndex], fenced by nInst, so a record the caller's aliasing of `hits` spoiled cannot make this
// kernel -- or k_shade after it, which reads insts[hitInst] -- read outside the instance array.
__global__ void __launch_bounds__(PATHS_INGEST_BLOCK)
k_paths_ingest(const uint32_t* __restrict__ slotOf, uint32_t nInst, const float4* __restrict__ rays, const float4* __restrict__ hits,
               const uint4* __restrict__ keys, uint32_t n, PathStreams ps)
{
    const uint32_t i = blockIdx.x * PATHS_INGEST_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 ro = rays[2 * (size_t)i], rd = rays[2 * (size_t)i + 1];
    const float4 ha = hits[2 * (size_t)i], hb = hits[2 * (size_t)i + 1];
    const uint4 key = keys[i];
    uint32_t slot = PATHS_MISS;
    if (__float_as_uint(ha.w) == 1u) {
        const uint32_t inst = __float_as_uint(hb.y);
        if (inst < nInst) slot = slotOf[inst];
        if (slot >= nInst) slot = PATHS_MISS;
    }
    ps.rayO[i] = make_float4(ro.x, ro.y, ro.z, __uint_as_float(key.y));
    ps.rayD[i] = make_float4(rd.x, rd.y, rd.z, __uint_as_float(key.x));
    ps.thr[i] = make_float4(1.0f, 1.0f, 1.0f, __uint_as_float(i));
    ps.col[i] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    ps.hitA[i] = make_float4(ha.x, ha.y, ha.z, hb.x);
    ps.hitInst[i] = slot;
}

void launch_paths_ingest(hipStream_t st, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits, const uint4* keys,
                         uint32_t n, const PathStreams& ps)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PATHS_INGEST_BLOCK - 1) / PATHS_INGEST_BLOCK);
    hipLaunchKernelGGL(k_paths_ingest, dim3(blocks), dim3(PATHS_INGEST_BLOCK), 0, st, slotOf, nInst, rays, hits, keys, n, ps);
}

} // namespace rdx

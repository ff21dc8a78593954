// surface.hip -- device side of rdx_resolve_hits: the surface record of a closest-hit ray query (include/rdx.h rdx_surface).
//
// A translation unit of its own, like tlas_update.hip and for the same reason: the code object of kernels.hip stays the one it
// was, bit for bit (profiles/surface_kernels.txt).  The arithmetic is the closest-hit shader's up to the offset origin
// (stages.h `material`, kernels.hip fill_hit_info), restated here so that neither is touched; device_math.h is shared.
#include "kernels.h"

#include "device_math.h"
#include "surface.h"

namespace rdx {

constexpr uint32_t RESOLVE_BLOCK = 256;

// One ray per thread: ray i = rays[2i], rays[2i + 1] (origin | tmin, direction | tmax), record i = hits[2i], hits[2i + 1]
// (t, b1, b2, hit | primitiveIndex, instanceIndex, customIndex, SBTOffset), surface i = out[4i .. 4i + 3]: adjacent lanes read
// adjacent 32-byte records and write adjacent 64-byte ones.  Dependent gathers of a hit: slotOf[instanceIndex] and
// MeshInfo[instanceIndex] (independent of each other), then 3 indices, then 9 normal + 6 uv floats and the instance's inv / fwd.
// Every gather is fenced by surface_in_bounds: a record that fails it writes zeros and is counted -- one ballot per wave, one
// atomic by its first lane, and only where the wave has such a record at all.
__global__ void __launch_bounds__(RESOLVE_BLOCK)
k_resolve_hits(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, const float4* __restrict__ rays,
               const float4* __restrict__ hits, uint32_t n, SurfaceScene sc, float4* __restrict__ out, uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * RESOLVE_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float4 ro = rays[2 * (size_t)i], rd = rays[2 * (size_t)i + 1];
        const float4 ha = hits[2 * (size_t)i], hb = hits[2 * (size_t)i + 1];
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
        if (__float_as_uint(ha.w) == 1u) {
            const uint32_t prim = __float_as_uint(hb.x), inst = __float_as_uint(hb.y);
            uint32_t slot = 0xffffffffu, idx[3] = {0u, 0u, 0u};
            bool ok = surface_in_bounds(sc.meshInfo, nInst, sc.nMeshInfo, inst, prim, nullptr, sc.nIndex, sc.nNormal, sc.nUv);
            if (ok) {
                slot = slotOf[inst];        // 0xffffffff: no instance of the TLAS carries this index (a foreign blob)
                const int64_t first = (int64_t)sc.meshInfo[inst].indexOffset + (int64_t)prim * 3;
                idx[0] = sc.index[first]; idx[1] = sc.index[first + 1]; idx[2] = sc.index[first + 2];
                ok = slot < nInst && surface_in_bounds(sc.meshInfo, nInst, sc.nMeshInfo, inst, prim, idx, sc.nIndex, sc.nNormal, sc.nUv);
            }
            if (ok) {
                const MeshInfo mi = sc.meshInfo[inst];
                const DInst& I = insts[slot];
                // HitData.hitPoint = localOrigin + localDir * t and barycentric, as kernels.hip fill_hit_info (radiance.cl:243)
                const f3 lo = mat4_mul3(I.inv, ro.x, ro.y, ro.z, 1.0f);
                const f3 ld = mat4_mul3(I.inv, rd.x, rd.y, rd.z, 0.0f);
                const f3 hp = lo + ld * ha.x;
                const float bx = 1 - ha.y - ha.z, by = ha.y, bz = ha.z;
                // getFaceNormal (samples/shader.cl:338-367): the interpolated vertex normal -> world by the object->world matrix,
                // w = 0, normalised; restated from stages.h:244-253
                const float* nb = sc.normal + (int64_t)mi.normalOffset;
                const int64_t v0 = (int64_t)idx[0] * 3, v1 = (int64_t)idx[1] * 3, v2 = (int64_t)idx[2] * 3;
                const f3 n0 = mk3(nb[v0], nb[v0 + 1], nb[v0 + 2]);
                const f3 n1 = mk3(nb[v1], nb[v1 + 1], nb[v1 + 2]);
                const f3 n2 = mk3(nb[v2], nb[v2 + 1], nb[v2 + 2]);
                const f3 nl = mk3(bx * n0.x + by * n1.x + bz * n2.x, bx * n0.y + by * n1.y + bz * n2.y, bx * n0.z + by * n1.z + bz * n2.z);
                const float nw = bx * 0.0f + by * 0.0f + bz * 0.0f;
                const f3 N = normalize3(mat4_mul3(I.fwd, nl.x, nl.y, nl.z, nw));
                // getHitPosition (shader.cl:453-468): transform * (hitPoint, 1), pushed off the surface along N and along -N
                const f3 P = mat4_mul3(I.fwd, hp.x, hp.y, hp.z, 1.0f);
                const f3 above = P + N * 0.00001f;
                const f3 below = P + (-N) * 0.00001f;
                // getUV (shader.cl:322-336)
                float u = 0.0f, v = 0.0f;
                if (sc.uv) {
                    const float* ub = sc.uv + (int64_t)mi.uvOffset;
                    u = bx * ub[v0] + by * ub[v1] + bz * ub[v2];
                    v = bx * ub[v0 + 1] + by * ub[v1 + 1] + bz * ub[v2 + 1];
                }
                r0 = make_float4(P.x, P.y, P.z, __uint_as_float(1u));
                r1 = make_float4(N.x, N.y, N.z, __uint_as_float((uint32_t)mi.materialIndex));
                r2 = make_float4(above.x, above.y, above.z, u);
                r3 = make_float4(below.x, below.y, below.z, v);
            } else {
                bad = true;
            }
        }
        float4* o = out + 4 * (size_t)i;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    }
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (uint32_t)__popcll(m));
}

void launch_resolve_hits(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits,
                         uint32_t n, const SurfaceScene& sc, float4* out, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + RESOLVE_BLOCK - 1) / RESOLVE_BLOCK);
    hipLaunchKernelGGL(k_resolve_hits, dim3(blocks), dim3(RESOLVE_BLOCK), 0, st, insts, slotOf, nInst, rays, hits, n, sc, out, invalid);
}

} // namespace rdx

// shade.hip -- device side of rdx_shade_hits: the stock closest-hit / miss shaders on the records of a ray query (include/rdx.h
// rdx_shade).
//
// A translation unit of its own, like surface.hip and tlas_update.hip and for the same reason: the code objects of kernels.hip and
// surface.hip stay the ones they were, bit for bit (profiles/shade_kernels.txt).  The shaders are those of stages.h, called through
// the generated SBT dispatch exactly as k_shade (kernels.hip) calls them; the HitInfo derivation is restated from surface.hip /
// kernels.hip fill_hit_info so that neither is touched.
#include "kernels.h"

#include "device_math.h"
#include "shade.h"
#include "stages.h"
#include "surface.h"

namespace rdx {

// 256 threads = 4 waves, no minimum-waves clause: the compiler's resource report (tools/kernel_resources.sh) shows
// `material` fitting without scratch at this bound, so a tighter register budget would only trade occupancy for spills
constexpr uint32_t SHADE_HITS_BLOCK = 256;

// One ray per thread: ray i = rays[2i], rays[2i + 1] (origin | tmin, direction | tmax), record i = hits[2i], hits[2i + 1] (t, b1, b2,
// hit | primitiveIndex, instanceIndex, customIndex, SBTOffset), key i = keys[i] (frameID, pixel, depth, -), shade record i =
// shade[3i .. 3i + 2]: adjacent lanes read and write adjacent records.  A surviving ray's next / shadow ray goes to record k of
// `next` / `shadow`: k = i, or -- `src` given -- the wave's base from ONE atomic on *live by its first lane plus the ray's rank in
// the wave's ballot, so the survivors of 64 consecutive inputs stay together and in input order.  *live counts the survivors
// either way.  Every gather of a hit is fenced by shade_in_bounds (shade.h); a record that fails it is zeroed and counted in
// *invalid like k_resolve_hits counts its own.
__global__ void __launch_bounds__(SHADE_HITS_BLOCK)
k_shade_hits(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, const float4* __restrict__ rays,
             const float4* __restrict__ hits, const uint4* __restrict__ keys, uint32_t n, ShadeScene sc, float4* __restrict__ shade,
             float4* __restrict__ next, float4* __restrict__ shadow, uint32_t* __restrict__ src, uint32_t* __restrict__ live,
             uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * SHADE_HITS_BLOCK + threadIdx.x;
    const bool active = i < n;
    bool bad = false, alive = false;
    Payload p;
    p.hit = false; p.wantsShadowRay = false;
    p.color = p.colorOccluded = p.nextFactor = p.nextRayOrigin = p.nextRayDirection = p.shadowOrigin = mk3(0.f, 0.f, 0.f);
    uint32_t materialIndex = 0u;
    f3 L = mk3(0.f, 0.f, 0.f);
    float tmaxShadow = 0.0f;       // a hit shader that asks for no shadow query: a shadow ray that accepts nothing
    if (active) {
        const float4 ro = rays[2 * (size_t)i], rd = rays[2 * (size_t)i + 1];
        const float4 ha = hits[2 * (size_t)i], hb = hits[2 * (size_t)i + 1];
        const uint4 key = keys[i];
        if (__float_as_uint(ha.w) == 1u) {
            const uint32_t prim = __float_as_uint(hb.x), inst = __float_as_uint(hb.y);
            const bool texOn = (sc.tex.flags & TEX_ENABLED) != 0u;
            uint32_t slot = 0xffffffffu, idx[3] = {0u, 0u, 0u};
            bool ok = shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, nullptr, sc.s.nIndex, sc.s.nNormal, sc.s.nUv, sc.materials,
                                      sc.nMaterials, texOn, sc.tex.layers);
            if (ok) {
                slot = slotOf[inst];        // 0xffffffff: no instance of the TLAS carries this index (a foreign blob)
                const int64_t first = (int64_t)sc.s.meshInfo[inst].indexOffset + (int64_t)prim * 3;
                idx[0] = sc.s.index[first]; idx[1] = sc.s.index[first + 1]; idx[2] = sc.s.index[first + 2];
                ok = slot < nInst && shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, idx, sc.s.nIndex, sc.s.nNormal, sc.s.nUv,
                                                     sc.materials, sc.nMaterials, texOn, sc.tex.layers);
            }
            if (ok) {
                const DInst& I = insts[slot];
                // HitData.hitPoint = localOrigin + localDir * t and barycentric, as kernels.hip fill_hit_info (radiance.cl:243)
                HitInfo h;
                const f3 lo = mat4_mul3(I.inv, ro.x, ro.y, ro.z, 1.0f);
                const f3 ld = mat4_mul3(I.inv, rd.x, rd.y, rd.z, 0.0f);
                h.hitPoint = lo + ld * ha.x;
                h.bx = 1 - ha.y - ha.z; h.by = ha.y; h.bz = ha.z;
                h.primitiveIndex = prim;
                h.instanceIndex = inst;
                h.fwd = I.fwd;
                const SceneView sv{sc.scene, sc.s.meshInfo, sc.s.index, sc.s.uv, sc.s.normal, sc.materials, sc.tex};
                // what a hit shader does not write keeps the payload's state on entry, which is k_shade's (shader.cl:208-214): factor
                // 1, the next ray = this ray, no shadow query
                p.nextFactor = mk3(1.f, 1.f, 1.f);
                p.nextRayOrigin = mk3(ro.x, ro.y, ro.z); p.nextRayDirection = mk3(rd.x, rd.y, rd.z);
                callHit((int)__float_as_uint(hb.w) + 1, p, h, sv, mk3(rd.x, rd.y, rd.z), key.x, key.y, key.z, next != nullptr);
                materialIndex = (uint32_t)sc.s.meshInfo[inst].materialIndex;
                alive = p.hit;
                if (!alive) p.nextFactor = mk3(0.f, 0.f, 0.f);      // (a table without a closest-hit shader in that row)
                if (alive && p.wantsShadowRay) {        // the shadow ray's direction, as `material` forms it (stages.h, shader.cl:489)
                    const float* d = sc.scene->lights[0].direction;
                    L = normalize3(mk3(-d[0], -d[1], -d[2]));
                    tmaxShadow = 1000.0f;
                }
            } else {
                bad = true;
            }
        } else {
            callMiss(3, p);
        }
    }
    // wave64 ballot: every lane of the wave is here (no thread has returned)
    const unsigned long long m = __ballot(alive), mb = __ballot(bad);
    const uint32_t lane = __lane_id();
    uint32_t base = 0u;
    if (m != 0ull) {
        if (lane == 0u) base = atomicAdd(live, (uint32_t)__popcll(m));
        base = (uint32_t)__builtin_amdgcn_readfirstlane((int)base);
    }
    if (mb != 0ull && lane == 0u) atomicAdd(invalid, (uint32_t)__popcll(mb));
    if (!active) return;
    const uint32_t k = src ? base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull)) : i;
    float4* o = shade + 3 * (size_t)i;
    if (bad) {
        o[0] = make_float4(0.f, 0.f, 0.f, 0.f); o[1] = o[0]; o[2] = make_float4(0.f, 0.f, 0.f, __uint_as_float(0xffffffffu));
    } else {
        o[0] = make_float4(p.color.x, p.color.y, p.color.z, __uint_as_float(p.hit ? 1u : 0u));
        o[1] = make_float4(p.colorOccluded.x, p.colorOccluded.y, p.colorOccluded.z, __uint_as_float(materialIndex));
        o[2] = make_float4(p.nextFactor.x, p.nextFactor.y, p.nextFactor.z, __uint_as_float(alive ? k : 0xffffffffu));
    }
    if (alive) {
        if (next) {
            next[2 * (size_t)k] = make_float4(p.nextRayOrigin.x, p.nextRayOrigin.y, p.nextRayOrigin.z, 0.001f);
            next[2 * (size_t)k + 1] = make_float4(p.nextRayDirection.x, p.nextRayDirection.y, p.nextRayDirection.z, 1000.0f);
        }
        if (shadow) {
            shadow[2 * (size_t)k] = make_float4(p.shadowOrigin.x, p.shadowOrigin.y, p.shadowOrigin.z, tmaxShadow != 0.0f ? 0.001f : 0.0f);
            shadow[2 * (size_t)k + 1] = make_float4(L.x, L.y, L.z, tmaxShadow);
        }
        if (src) src[k] = i;
    } else if (!src) {      // not compacting: record i of a ray that does not survive is a ray that accepts nothing (tmax = 0)
        const float4 z = make_float4(0.f, 0.f, 0.f, 0.f);
        if (next) { next[2 * (size_t)i] = z; next[2 * (size_t)i + 1] = z; }
        if (shadow) { shadow[2 * (size_t)i] = z; shadow[2 * (size_t)i + 1] = z; }
    }
}

void launch_shade_hits(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits,
                       const uint4* keys, uint32_t n, const ShadeScene& sc, float4* shade, float4* next, float4* shadow, uint32_t* src,
                       uint32_t* live, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + SHADE_HITS_BLOCK - 1) / SHADE_HITS_BLOCK);
    hipLaunchKernelGGL(k_shade_hits, dim3(blocks), dim3(SHADE_HITS_BLOCK), 0, st, insts, slotOf, nInst, rays, hits, keys, n, sc, shade, next,
                       shadow, src, live, invalid);
}

} // namespace rdx

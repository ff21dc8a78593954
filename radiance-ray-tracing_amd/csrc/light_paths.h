// light_paths.h -- launch declarations of rdx_trace_paths_lights (light_paths.hip): one bounce of a path tracer over every
// directional light of the scene, as two kernels around the any-hit query of the bounce's shadow rays.  The scene view and the
// bounds rule are those of rdx_shade_hits (shade.h: ShadeScene, shade_in_bounds), unchanged.
#pragma once
#include <stdint.h>

#include "rdx_types.h"
#include "shade.h"

namespace rdx {

#if defined(__HIPCC__)
// The streams of one bounce.  A LIVE RAY k of depth d is record k of rays / hits / ids / weight; a SURVIVOR k' of depth d -- a
// live ray with a valid hit -- is live ray k' of depth d + 1, so the n* streams of one bounce are the plain ones of the next (the
// host swaps the pointers).  L = the call's light_count.
struct LightPathStreams {
    const float4* rays;      // 2 per live ray: origin | tmin, direction | tmax
    const float4* hits;      // 2 per live ray: its closest-hit query record
    const uint4* keys;       // depth 0 only: the caller's keys (path = ray number, frameID, pixel from the key, weight 1); else null
    const uint4* ids;        // depth > 0: path number, frameID, pixel, 0 per live ray
    const float4* weight;    // depth > 0: weight.xyz per live ray
    uint4* nIds;             // per survivor: the ids of its path
    float4* nWeight;         // per survivor: k_lights_shade copies the weight, k_lights_fold multiplies it by nextFactor
    float4* nRays;           // per survivor: the next ray (not written when the next direction is not sampled)
    float4* foldF;           // per survivor: nextFactor | 0
    float4* foldA;           // per survivor: albedo * 0.1f | 0
    float4* lit;             // record k' * L + j: light j's direct term (rgb, 0)
    float4* shadow;          // records 2 * (k' * L + j), + 1: the shadow ray towards light j -- one contiguous range per bounce
    float4* radiance;        // the chunk's part of the caller's radiance range, by path number
};

// k_lights_shade: n live rays of depth `depth`.  *live (zero before the launch) += survivors and is the compaction cursor,
// *invalid += hits that fail shade_in_bounds or whose instance no slot carries.  At depth 0 radiance[path] is written for every
// path: zeros, or the miss colour.  sampleNext = false (the last depth): no next direction, nRays and foldF.xyz are not meaningful.
void launch_lights_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const DirLight* lights,
                         uint32_t nLights, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext, uint32_t* live,
                         uint32_t* invalid);
// k_lights_fold: `live` survivors; any = the RDX_QUERY_ANY records of io.shadow (2 per shadow ray; not read when nLights is 0).
// direct = sum over j in order of (occluded ? 0 : lit_j); radiance[path] += weight * (direct + ambient); weight *= nextFactor.
void launch_lights_fold(hipStream_t st, const float4* any, uint32_t nLights, const LightPathStreams& io, uint32_t live);
#endif

} // namespace rdx

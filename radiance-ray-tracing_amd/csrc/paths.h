// paths.h -- launch interface of rdx_trace_paths (paths.hip): the caller's rays enter the frame path's streams.  All pointers are
// device pointers; the launch goes to the given stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace rdx {

// One lane per path: ray i = rays[2i], rays[2i + 1] (origin | tmin, direction | tmax), the closest-hit record of its first segment
// = hits[2i], hits[2i + 1] (rdx_ray_hit), key i = keys[i] (frameID, pixel, -, -) become path i of `ps` as k_generate and
// extend(0) of the frame path leave it: rayO = (origin | pixel), rayD = (direction | frameID), thr = (1, 1, 1 | i), col = 0,
// hitA = (t, b1, b2 | primitiveIndex), hitInst = slotOf[instanceIndex], or 0xffffffff (a miss) for a record whose `hit` is not 1,
// whose instanceIndex is not below nInst or has no slot.  slotOf: nInst words (AccelCache::slotOf).
void launch_paths_ingest(hipStream_t st, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits, const uint4* keys,
                         uint32_t n, const PathStreams& ps);

} // namespace rdx

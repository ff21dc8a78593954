// temporal.h -- the records and the launch declarations of rdx_camera_view and rdx_temporal_accumulate (temporal.hip): the temporal
// half of SVGF (Schied et al. 2017) -- a frame's history reprojected through the previous view, tested for consistency against the
// history's own guide, folded into an exponential mean of the colour and of the first two luminance moments, with a per-pixel
// variance estimate (include/rdx.h).  A history is four planes of one float4 per pixel, 64 bytes per pixel:
//
//   plane 0 [W H] = (rgb | w: the bits of the current colour's)      what rdx_denoise takes as `color`, at offset 0, without a copy
//   plane 1 [W H] = (m1 | m2 | variance | N)                         N: the history length, a uint32
//   plane 2 [W H] = (n.xyz | materialIndex)
//   plane 3 [W H] = (P.xyz | valid)                                  1u or 0u
//
// Planes, not records: a wave's tap is then a contiguous row of float4 per plane.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rdx {

constexpr uint32_t TEMPORAL_MAX_DIM = 16384u;          // width and height: the limits of rdx_denoise
constexpr uint32_t TEMPORAL_MAX_PIXELS = 1u << 26;
constexpr uint32_t TEMPORAL_MAX_HISTORY = 65535u, TEMPORAL_MAX_VARIANCE_HISTORY = 255u;
constexpr uint32_t TEMPORAL_DEBUG = 1u;                // rdx_temporal_settings.flags
constexpr uint32_t TEMPORAL_POSITION = 2u;             // TemporalArgs.flags only: the position term is on

// 0: a size outside the limits
inline size_t temporal_history_size(uint32_t w, uint32_t h)
{
    if (w < 1u || w > TEMPORAL_MAX_DIM || h < 1u || h > TEMPORAL_MAX_DIM || (uint64_t)w * h > TEMPORAL_MAX_PIXELS) return 0;
    return (size_t)w * h * 64u;
}

// what the host hands to both launches of a call
struct TemporalArgs {
    uint32_t W, H;
    uint32_t maxHistory, varianceMinHistory, flags;
    float alphaMin, alphaMomentsMin, normalCosMin, positionTolerance;
};

#if defined(__HIPCC__)
struct PhysicalCamera;
// *view = the rdx_view of the camera buffer's current contents.  One thread
void launch_camera_view(hipStream_t st, const PhysicalCamera* camera, float4* view);
// rdx_temporal_accumulate after the host's checks: k_temporal_reproject, then (varianceMinHistory != 0) k_temporal_variance in stream
// order.  previousPositions, historyIn and image may be null; previousView is never null (the host passes view for an absent one)
void launch_temporal_accumulate(hipStream_t st, const TemporalArgs& a, const float4* color, const float4* materials, const float4* surfaces,
                                const float4* previousPositions, const float4* view, const float4* previousView, const float4* historyIn, float4* historyOut,
                                uchar4* image);
#endif

} // namespace rdx

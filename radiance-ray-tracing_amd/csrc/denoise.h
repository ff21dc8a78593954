// denoise.h -- the records and the launch declaration of rdx_denoise (denoise.hip): an edge-avoiding a-trous wavelet filter
// (Dammertz et al. 2010) over a W x H image of float4 colours, guided by the rdx_material_record and rdx_surface records of the
// same pixels' primary hits (include/rdx.h).  The caller's work range holds three planes of one float4 per pixel:
//
//   iterate[W H] | guideN[W H] = (n.xyz | valid) | guideP[W H] = (P.xyz | 0)          48 bytes per pixel
//
// The guide is the packed 32 bytes a tap needs of the two 64-byte records, as two planes: a wave's tap is then two contiguous
// 1 KiB rows.  The iterates alternate between the work range and the caller's `out`, so that the last pass lands in `out`.
#pragma once
#include <stddef.h>
#include <stdint.h>

namespace rdx {

constexpr uint32_t DENOISE_MAX_DIM = 16384u;           // width and height
constexpr uint32_t DENOISE_MAX_PIXELS = 1u << 26;
constexpr uint32_t DENOISE_MAX_PASSES = 8u, DENOISE_MAX_SQUARINGS = 7u;
constexpr uint32_t DENOISE_DEMODULATE = 1u, DENOISE_DEBUG = 2u;        // rdx_denoise_settings.flags
constexpr uint32_t DENOISE_POSITION = 4u, DENOISE_COLOUR = 8u;         // DenoiseArgs.flags only: the term is on

// 0: a size outside the limits
inline size_t denoise_work_size(uint32_t w, uint32_t h)
{
    if (w < 1u || w > DENOISE_MAX_DIM || h < 1u || h > DENOISE_MAX_DIM || (uint64_t)w * h > DENOISE_MAX_PIXELS) return 0;
    return (size_t)w * h * 48u;
}

// what the host hands to every launch of a call
struct DenoiseArgs {
    uint32_t W, H;
    uint32_t passes, squarings, flags;
    float sigmaPosition, sigmaColour;
    uint32_t tiled;             // bit j: pass j (step 1 << j, j < 2) takes its taps from an LDS tile; 3 unless rdx_debug_denoise_tiled changed it
};

#if defined(__HIPCC__)
// rdx_denoise after the host's checks: prepare, then `passes` passes in stream order, the last one (or, with no pass, prepare)
// fused with the finish.  image may be null.
void launch_denoise(hipStream_t st, const DenoiseArgs& a, const float4* color, const float4* materials, const float4* surfaces, float4* work, float4* out,
                    uchar4* image);
#endif

} // namespace rdx

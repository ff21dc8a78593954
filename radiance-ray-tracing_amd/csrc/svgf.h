// svgf.h -- the records and the launch declaration of rdx_svgf_filter (svgf.hip): the variance-guided a-trous filter of SVGF
// (Schied et al. 2017) over a W x H image of float4 colours and the per-pixel luminance variance rdx_temporal_accumulate
// estimates, guided by the rdx_material_record and rdx_surface records of the same pixels' primary hits (include/rdx.h;
// DESIGN 4.21).  The caller's work range holds three planes of one float4 per pixel, the layout of rdx_denoise's:
//
//   iterate[W H] = (i.rgb | v) | guideN[W H] = (n.xyz | valid) | guideP[W H] = (P.xyz | 0)          48 bytes per pixel
//
// The variance rides in the iterate's w, so a tap stays three float4 loads; color[p].w is read again where `out` and `feedback`
// are written.  The iterates alternate between the work range and the caller's `out`, so that the last pass lands in `out`.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include "denoise.h"

namespace rdx {

constexpr uint32_t SVGF_LUMINANCE = 8u;                // SvgfArgs.flags only, beside DENOISE_POSITION: the term is on

// 0: a size outside the limits of denoise_work_size
inline size_t svgf_work_size(uint32_t w, uint32_t h) { return denoise_work_size(w, h); }

// what the host hands to every launch of a call
struct SvgfArgs {
    uint32_t W, H;
    uint32_t passes, squarings, flags;
    float sigmaPosition, sigmaLuminance, epsilon;
    uint32_t feedbackPass;      // 0, or 1 .. passes: the pass after which `feedback` is written
    uint32_t tiled;             // bit j: pass j (step 1 << j, j < 2) takes its taps from an LDS tile; rdx_debug_svgf_tiled sets it
};

#if defined(__HIPCC__)
// rdx_svgf_filter after the host's checks: prepare, then `passes` passes in stream order, the last one (or, with no pass, prepare)
// fused with the finish.  variance_out, feedback (given iff feedbackPass != 0) and image may be null.
void launch_svgf_filter(hipStream_t st, const SvgfArgs& a, const float4* color, const float4* moments, const float4* materials, const float4* surfaces,
                        float4* work, float4* out, float* variance_out, float4* feedback, uchar4* image);
#endif

} // namespace rdx

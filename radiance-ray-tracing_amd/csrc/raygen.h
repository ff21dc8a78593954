// raygen.h -- launch interface of rdx_generate_rays / rdx_accumulate (raygen.hip): the two ends of a frame on the public record
// formats of include/rdx.h.  All pointers are device pointers; all launches go to the given stream.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

#include "kernels.h"

namespace rdx {

// rdx_generate_rays.  First one thread turns the PhysicalCamera at `camera` into the CameraArgs at `args` -- cos / sin of the
// three angles with the OCML functions, the matrices camera_args (rdx_runtime.cpp) builds from them -- then one lane per ray
// writes ray i = generateRay(pixel_i, pcg3d(seed_i)) with (tmin, tmax) to rays[2i], rays[2i + 1] and, `keys` given, (frameID,
// pixel_i, 0, 0) to keys[i].  pixel_i = pixels ? pixels[i] : firstPixel + i; seed_i = seeds ? seeds[i].xyz : (frameID,
// totalSamples, pixel_i).  `args` is device memory of the runtime's own, rewritten by every call.
void launch_generate_rays(hipStream_t st, const PhysicalCamera* camera, CameraArgs* args, uint32_t n, uint32_t firstPixel,
                          const uint32_t* pixels, uint32_t frameID, uint32_t totalSamples, const uint4* seeds, float tmin, float tmax,
                          float4* rays, uint4* keys);

// rdx_accumulate.  One lane per sample: colors[i].xyz is folded into scratch[pixel_i].xyz as sample `frameID` of the running
// mean (w kept) and, `image` given, image[pixel_i] becomes the tone-mapped mean.  A pixel_i >= nPixels writes nothing and
// is counted in *invalid.
void launch_accumulate_samples(hipStream_t st, const float4* colors, uint32_t n, uint32_t firstPixel, const uint32_t* pixels,
                               uint32_t frameID, float4* scratch, uchar4* image, uint32_t nPixels, uint32_t debug, uint32_t* invalid);

} // namespace rdx

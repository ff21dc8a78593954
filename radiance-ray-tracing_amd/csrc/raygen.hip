// raygen.hip -- device side of rdx_generate_rays and rdx_accumulate: the two ends of a frame on the public record formats
// (include/rdx.h rdx_ray, rdx_shade_key, rdx_raygen_seed; imageScratch and the RGBA8 image of descriptor slots 1 and 2).
//
// A translation unit of its own, like shade.hip, surface.hip and tlas_update.hip: the frame path's kernels stay in kernels.hip.
// The arithmetic is not restated here -- camera_ray, pcg3d, fold_sample and store_rgba8 are the device functions k_generate /
// k_accumulate call (raygen_device.h, device_math.h).
#include "raygen.h"

#include "device_math.h"
#include "raygen_device.h"

namespace rdx {

constexpr uint32_t RAYGEN_BLOCK = 256;

// The per-call constants of generateRay, from the camera buffer's CURRENT contents: EulerX/Y/ZToMat4x4 (math.cl:185-252) with the
// OCML cos / sin of k_euler_trig (kernels.hip), laid out as camera_args (rdx_runtime.cpp) lays them out.  One thread.
__global__ void k_raygen_camera(const PhysicalCamera* __restrict__ camera, CameraArgs* __restrict__ args)
{
    const PhysicalCamera cam = *camera;
    const float cx = cosf(cam.wx), sx = sinf(cam.wx), cy = cosf(cam.wy), sy = sinf(cam.wy), cz = cosf(cam.wz), sz = sinf(cam.wz);
    const float rx[16] = {1, 0, 0, 0, 0, cx, -sx, 0, 0, sx, cx, 0, 0, 0, 0, 1};
    const float ry[16] = {cy, 0, sy, 0, 0, 1, 0, 0, -sy, 0, cy, 0, 0, 0, 0, 1};
    const float rz[16] = {cz, -sz, 0, 0, sz, cz, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    args->cam = cam;
    for (int k = 0; k < 16; ++k) { args->rotX[k] = rx[k]; args->rotY[k] = ry[k]; args->rotZ[k] = rz[k]; }
}

// One ray per lane: adjacent lanes read adjacent pixels / seeds and write adjacent records -- the 32-byte ray as two 16-byte
// stores, the 16-byte key as one.  The pixel number only enters arithmetic, never an address.  No LDS, no atomics.
__global__ void __launch_bounds__(RAYGEN_BLOCK)
k_generate_rays(const CameraArgs* __restrict__ args, uint32_t n, uint32_t firstPixel, const uint32_t* __restrict__ pixels,
                uint32_t frameID, uint32_t totalSamples, const uint4* __restrict__ seeds, float tmin, float tmax,
                float4* __restrict__ rays, uint4* __restrict__ keys)
{
    const uint32_t i = blockIdx.x * RAYGEN_BLOCK + threadIdx.x;
    if (i >= n) return;
    const uint32_t pixel = pixels ? pixels[i] : firstPixel + i;
    uint4 seed = make_uint4(frameID, totalSamples, pixel, 0u);      // shader.cl:205
    if (seeds) seed = seeds[i];
    const f3 rnd = pcg3d(seed.x, seed.y, seed.z);
    f3 o, d;
    camera_ray(*args, pixel, rnd, o, d);
    rays[2 * (size_t)i] = make_float4(o.x, o.y, o.z, tmin);
    rays[2 * (size_t)i + 1] = make_float4(d.x, d.y, d.z, tmax);
    if (keys) keys[i] = make_uint4(frameID, pixel, 0u, 0u);
}

// One sample per lane: a 16-byte load of the colour, a 16-byte load and store of the pixel's imageScratch value, a 4-byte store
// of its RGBA8.  The pixel number IS an address here: one not below nPixels touches nothing and is counted, one atomic per
// wave that holds such a sample (none otherwise).  Two samples of one pixel in a call race; each access stays inside the buffers.
__global__ void __launch_bounds__(RAYGEN_BLOCK)
k_accumulate_samples(const float4* __restrict__ colors, uint32_t n, uint32_t firstPixel, const uint32_t* __restrict__ pixels,
                     uint32_t frameID, float4* __restrict__ scratch, uchar4* __restrict__ image, uint32_t nPixels, uint32_t debug,
                     uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * RAYGEN_BLOCK + threadIdx.x;
    const bool active = i < n;
    uint32_t pixel = 0u;
    if (active) pixel = pixels ? pixels[i] : firstPixel + i;
    const bool bad = active && pixel >= nPixels;
    // wave64 ballot: every lane of the wave is here (no thread has returned)
    const unsigned long long mb = __ballot(bad);
    if (mb != 0ull && __lane_id() == 0u) atomicAdd(invalid, (uint32_t)__popcll(mb));
    if (!active || bad) return;
    float4 acc = scratch[pixel];
    fold_sample(acc, colors[i], frameID);
    scratch[pixel] = acc;
    if (image) store_rgba8(image + pixel, mk3(acc.x, acc.y, acc.z), debug);
}

void launch_generate_rays(hipStream_t st, const PhysicalCamera* camera, CameraArgs* args, uint32_t n, uint32_t firstPixel,
                          const uint32_t* pixels, uint32_t frameID, uint32_t totalSamples, const uint4* seeds, float tmin, float tmax,
                          float4* rays, uint4* keys)
{
    if (!n) return;
    hipLaunchKernelGGL(k_raygen_camera, dim3(1), dim3(1), 0, st, camera, args);
    const uint32_t blocks = (uint32_t)(((uint64_t)n + RAYGEN_BLOCK - 1) / RAYGEN_BLOCK);
    hipLaunchKernelGGL(k_generate_rays, dim3(blocks), dim3(RAYGEN_BLOCK), 0, st, args, n, firstPixel, pixels, frameID, totalSamples, seeds,
                       tmin, tmax, rays, keys);
}

void launch_accumulate_samples(hipStream_t st, const float4* colors, uint32_t n, uint32_t firstPixel, const uint32_t* pixels,
                               uint32_t frameID, float4* scratch, uchar4* image, uint32_t nPixels, uint32_t debug, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + RAYGEN_BLOCK - 1) / RAYGEN_BLOCK);
    hipLaunchKernelGGL(k_accumulate_samples, dim3(blocks), dim3(RAYGEN_BLOCK), 0, st, colors, n, firstPixel, pixels, frameID, scratch, image,
                       nPixels, debug, invalid);
}

} // namespace rdx

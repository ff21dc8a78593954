// raygen_device.h -- the device functions of the two ends of a frame, shared by the frame path (kernels.hip: k_generate,
// k_generate_batch, k_path, k_accumulate) and by rdx_generate_rays / rdx_accumulate (raygen.hip): generateRay of the reference,
// the running mean of imageScratch and the tone map of the RGBA8 image.  One text for both units, so both give the same bits.
#pragma once
#include "device_math.h"
#include "kernels.h"
#include "stages.h"

namespace rdx {

// ---------------------------------------------------------------------------------------------
// generate: primary rays (samples/shader.cl:111-173, 196-231)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ void camera_ray(const CameraArgs& C, uint32_t pixel, f3 rnd, f3& org, f3& dir)
{
    const PhysicalCamera& cam = C.cam;
    const int index = (int)pixel;
    const int x = index % (int)cam.widthPixel;
    const int y = index / (int)cam.widthPixel;
    const float fx = (((float)x + rnd.x) / cam.widthPixel) - 0.5f;
    const float fy = 0.5f - (((float)y + rnd.y) / cam.heightPixel);
    const float aspect = cam.heightPixel / cam.widthPixel;
    f4 pd; pd.x = fx * cam.sensorWidth; pd.y = fy * cam.sensorWidth * aspect; pd.z = -cam.focalLength; pd.w = 0.0f;
    pd = normalize4(pd);
    const f3 eye = mk3(cam.x, cam.y, cam.z);
    const float time = -cam.focalDistance / pd.z;
    f4 t = mat4_mul(C.rotZ, pd.x, pd.y, pd.z, pd.w);
    pd = mat4_mul(C.rotY, t.x, t.y, t.z, t.w);
    t = mat4_mul(C.rotX, pd.x, pd.y, pd.z, pd.w);
    pd = normalize4(t);
    if (cam.fStop == 0.0f) { org = eye; dir = mk3(pd.x, pd.y, pd.z); return; }

    // thin lens: concentric disk sample from rnd.yz (shader.cl:89-109, 155-172)
    const float lensRadius = (cam.focalLength / cam.fStop) / 2.0f;
    float ux = 2.0f * rnd.y - 1.0f, uy = 2.0f * rnd.z - 1.0f;
    float lx = 0.0f, ly = 0.0f;
    if (!(ux == 0.0f && uy == 0.0f)) {
        float theta, rr;
        if (fabsf(ux) > fabsf(uy)) { rr = ux; theta = (RDX_PI / 4.0f) * (uy / ux); }
        else { rr = uy; theta = (RDX_PI / 2.0f) - (RDX_PI / 4.0f) * (ux / uy); }
        lx = rr * cosf(theta); ly = rr * sinf(theta);
    }
    lx = lensRadius * lx; ly = lensRadius * ly;
    const f3 focus = eye + mk3(pd.x, pd.y, pd.z) * time;
    f4 l = mat4_mul(C.rotZ, lx, ly, 0.0f, 1.0f);
    f4 l2 = mat4_mul(C.rotY, l.x, l.y, l.z, l.w);
    l = mat4_mul(C.rotX, l2.x, l2.y, l2.z, l2.w);
    org = eye + mk3(l.x, l.y, l.z);
    dir = normalize3(focus - org);
}

// ---------------------------------------------------------------------------------------------
// accumulate: running mean in sample order + ACES/gamma + RGBA8 (samples/shader.cl:262-304)
// ---------------------------------------------------------------------------------------------
__device__ __forceinline__ float aces1(float v)
{
    v = v * 0.6f;
    return cl_clamp((v * (2.51f * v + 0.03f)) / (v * (2.43f * v + 0.59f) + 0.14f), 0.0f, 1.0f);
}

// one sample `c` of frame `frameID` folded into the pixel's imageScratch value `acc` (shader.cl:262-270); acc.w is not touched
__device__ __forceinline__ void fold_sample(float4& acc, const float4& c, uint32_t frameID)
{
    if (frameID == 0) { acc.x = c.x; acc.y = c.y; acc.z = c.z; }
    else {
        acc.x = (frameID * acc.x + c.x) / (frameID + 1);
        acc.y = (frameID * acc.y + c.y) / (frameID + 1);
        acc.z = (frameID * acc.z + c.z) / (frameID + 1);
    }
}

// *dst = the RGBA8 pixel of the mean `c` (shader.cl:272-304); debug = RTProp.debug: no ACES, no gamma
__device__ __forceinline__ void store_rgba8(uchar4* dst, f3 c, uint32_t debug)
{
    if (!debug) {
        c = mk3(aces1(c.x), aces1(c.y), aces1(c.z));
        c = mk3(powf(c.x, 0.7f), powf(c.y, 0.7f), powf(c.z, 0.7f));
    }
    uchar4 o;
    o.x = (unsigned char)(int)(c.x * 255);
    o.y = (unsigned char)(int)(c.y * 255);
    o.z = (unsigned char)(int)(c.z * 255);
    o.w = 255;
    *dst = o;
}

} // namespace rdx

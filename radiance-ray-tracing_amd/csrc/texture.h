// texture.h -- the texture array sampler, shared by the stock closest-hit shader (stages.h, option "textures") and user shader
// programs (user_texture.hip, linked into the run-time compiled program by user_shader.cpp).  Device code here may use only
// operations that lower to LLVM instructions or intrinsics (__builtin_floorf / rintf / fabsf): user_texture.hip is linked
// into a user program by a final step that links no device library.
#pragma once
#include <hip/hip_runtime.h>
#include <stdint.h>

namespace rdx {

// descriptor slots 11 + 12: the RGBA8 texture array and its sampler (radiance.cpp:96-137; read by the commented-out
// read_imageui calls of samples/shader.cl:379-445, live in shader2.cl:255-265).  flags = 0: the stock pipeline behaves
// like the LIVE reference shader, whose texture reads are stubbed to 0.
enum : uint32_t { TEX_ENABLED = 1u, TEX_LINEAR = 2u, TEX_ADDR_SHIFT = 4u,      // flags
                  TEX_ADDR_REPEAT = 0u, TEX_ADDR_CLAMP_TO_EDGE = 1u, TEX_ADDR_CLAMP = 2u, TEX_ADDR_MIRRORED = 3u };
struct TexView { const uint8_t* data; uint32_t w, h, layers, flags; };

// what a user program's image2d_array_t / sampler_t parameters point to (user_texture.hip; filled by rdx_runtime.cpp
// user_tex_views).  A zero view stands for a NULL slot: reads return (0, 0, 0, 0), queries 0.
struct TexImageView { const uint8_t* data; uint32_t w, h, layers, pad; };
struct TexSamplerView { uint32_t flags, pad[3]; };            // flags as TexView::flags; 0 = no sampler

// ---- texture array reads -------------------------------------------------------------------------------------------
// read_imageui(imageArray, sampler, (float4)(u, v, layer, 0)) on a CL_RGBA / CL_UNSIGNED_INT8 2D image array with a
// normalized-coordinate sampler, per the OpenCL 1.2 specification, section 8.2 (addressing modes) and 5.3.3 (array layer =
// clamp(rint(layer), 0, layers - 1)).  The specification leaves CLK_FILTER_LINEAR undefined for integer reads; the
// reference binds a linear sampler (tools/sceneBuilder.cpp:40), so linear is DEFINED here as the spec's bilinear weights on
// the 8-bit values, rounded to nearest.  The live reference shader never reaches this code ("parity unpinned").
__device__ inline int tex_addr(float s, int n, uint32_t mode, float& u)          // -> nearest texel index (or -1: border), u = unnormalised
{
    if (mode == TEX_ADDR_REPEAT) { u = (s - __builtin_floorf(s)) * (float)n; int i = (int)__builtin_floorf(u); return i > n - 1 ? i - n : i; }
    if (mode == TEX_ADDR_MIRRORED) { float sp = 2.0f * __builtin_rintf(0.5f * s); sp = __builtin_fabsf(s - sp); u = sp * (float)n; int i = (int)__builtin_floorf(u); return i > n - 1 ? n - 1 : i; }
    u = s * (float)n;
    const int i = (int)__builtin_floorf(u);
    if (mode == TEX_ADDR_CLAMP_TO_EDGE) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    return (i < 0 || i > n - 1) ? -1 : i;                                          // CLAMP: border colour (0, 0, 0, 0)
}
__device__ inline int tex_wrap(int i, int n, uint32_t mode)                       // neighbour index of the linear filter
{
    if (mode == TEX_ADDR_REPEAT) return i < 0 ? i + n : (i > n - 1 ? i - n : i);
    if (mode == TEX_ADDR_MIRRORED || mode == TEX_ADDR_CLAMP_TO_EDGE) return i < 0 ? 0 : (i > n - 1 ? n - 1 : i);
    return (i < 0 || i > n - 1) ? -1 : i;
}
__device__ inline void tex_texel(const TexView& T, int layer, int x, int y, float out[4])
{
    if (x < 0 || y < 0) { out[0] = out[1] = out[2] = out[3] = 0.0f; return; }
    const uchar4 t = reinterpret_cast<const uchar4*>(T.data)[((size_t)layer * T.h + (uint32_t)y) * T.w + (uint32_t)x];
    out[0] = (float)t.x; out[1] = (float)t.y; out[2] = (float)t.z; out[3] = (float)t.w;
}
__device__ inline void tex_read_ui(const TexView& T, float u, float v, float layerF, uint32_t out[4])
{
    const uint32_t mode = (T.flags >> TEX_ADDR_SHIFT) & 3u;
    int layer = (int)__builtin_rintf(layerF);
    layer = layer < 0 ? 0 : (layer > (int)T.layers - 1 ? (int)T.layers - 1 : layer);
    float uu, vv;
    const int ix = tex_addr(u, (int)T.w, mode, uu), iy = tex_addr(v, (int)T.h, mode, vv);
    float c[4];
    if (!(T.flags & TEX_LINEAR)) {
        tex_texel(T, layer, ix, iy, c);
        for (int k = 0; k < 4; ++k) out[k] = (uint32_t)c[k];
        return;
    }
    const float fu = uu - 0.5f, fv = vv - 0.5f;
    const int i0 = (int)__builtin_floorf(fu), j0 = (int)__builtin_floorf(fv);
    const float a = fu - __builtin_floorf(fu), b = fv - __builtin_floorf(fv);
    const int x0 = tex_wrap(i0, (int)T.w, mode), x1 = tex_wrap(i0 + 1, (int)T.w, mode);
    const int y0 = tex_wrap(j0, (int)T.h, mode), y1 = tex_wrap(j0 + 1, (int)T.h, mode);
    float t00[4], t10[4], t01[4], t11[4];
    tex_texel(T, layer, x0, y0, t00); tex_texel(T, layer, x1, y0, t10); tex_texel(T, layer, x0, y1, t01); tex_texel(T, layer, x1, y1, t11);
    for (int k = 0; k < 4; ++k)
        out[k] = (uint32_t)((1.0f - a) * (1.0f - b) * t00[k] + a * (1.0f - b) * t10[k] + (1.0f - a) * b * t01[k] + a * b * t11[k] + 0.5f);
}

} // namespace rdx

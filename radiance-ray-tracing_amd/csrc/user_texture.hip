// user_texture.hip -- texture reads for user shader programs.  build.py compiles this file to device bitcode
// (user_texture.bc next to librdx.so); the run-time compiler (user_shader.cpp) links it into every user program, whose
// read_imageui / get_image_* calls on the bound texture array reach the functions below through its prelude and entry unit.
// The views are passed as 64-bit integers and the vectors as clang vector types, so that the calls match OpenCL C's
// `ulong`, `float4`, `int4` and `uint4` in the linked IR.  Only LLVM builtins here: the user program's final link step links no
// device library.
#include "texture.h"

using namespace rdx;

typedef float rdx_float4 __attribute__((ext_vector_type(4)));
typedef int rdx_int4 __attribute__((ext_vector_type(4)));
typedef unsigned rdx_uint4 __attribute__((ext_vector_type(4)));

namespace {

__device__ inline const TexImageView& image_of(uint64_t v) { return *reinterpret_cast<const TexImageView*>(v); }
__device__ inline bool empty(const TexImageView& I) { return !I.data || !I.w || !I.h || !I.layers; }

// coordinates that leave no doubt about the integer conversions of tex_addr / tex_read_ui: NaN reads as -2^24, and
// magnitudes beyond 2^24 are clamped there.  Floats that large are integers, so every addressing mode maps them to the
// texel it maps 2^24 to (repeat, mirrored repeat) or to the same edge / border texel.
__device__ inline float coord(float s) { return __builtin_fminf(__builtin_fmaxf(s, -16777216.0f), 16777216.0f); }

} // namespace

// read_imageui(image2d_array_t, sampler_t, float4): the stock shader's sampler (texture.h); a zero image or sampler view -> 0
extern "C" __device__ rdx_uint4 rdx_tex_read_sampled(uint64_t image, uint64_t sampler, rdx_float4 c)
{
    const TexImageView I = image_of(image);
    const uint32_t flags = reinterpret_cast<const TexSamplerView*>(sampler)->flags;
    rdx_uint4 r = {0u, 0u, 0u, 0u};
    if (empty(I) || !(flags & TEX_ENABLED)) return r;
    const TexView T{I.data, I.w, I.h, I.layers, flags};
    uint32_t out[4];
    tex_read_ui(T, coord(c.x), coord(c.y), coord(c.z), out);
    r.x = out[0]; r.y = out[1]; r.z = out[2]; r.w = out[3];
    return r;
}

// read_imageui(image2d_array_t, int4): texel (x, y) of layer z; out of range (or a zero view) -> 0
extern "C" __device__ rdx_uint4 rdx_tex_read_texel(uint64_t image, rdx_int4 c)
{
    const TexImageView I = image_of(image);
    rdx_uint4 r = {0u, 0u, 0u, 0u};
    if (empty(I) || c.x < 0 || c.y < 0 || c.z < 0 || (uint32_t)c.x >= I.w || (uint32_t)c.y >= I.h || (uint32_t)c.z >= I.layers) return r;
    const uchar4 t = reinterpret_cast<const uchar4*>(I.data)[((size_t)c.z * I.h + (uint32_t)c.y) * I.w + (uint32_t)c.x];
    r.x = t.x; r.y = t.y; r.z = t.z; r.w = t.w;
    return r;
}

extern "C" __device__ unsigned rdx_tex_width(uint64_t image) { const TexImageView I = image_of(image); return empty(I) ? 0u : I.w; }
extern "C" __device__ unsigned rdx_tex_height(uint64_t image) { const TexImageView I = image_of(image); return empty(I) ? 0u : I.h; }
extern "C" __device__ unsigned rdx_tex_layers(uint64_t image) { const TexImageView I = image_of(image); return empty(I) ? 0u : I.layers; }

// denoise.hip -- device side of rdx_denoise (include/rdx.h): an edge-avoiding a-trous wavelet filter over an image of
// float4 colours, guided by the primary hits' material and surface records --
//
//   k_denoise_prepare      one pixel per lane: the first iterate (the colour, divided by the clamped albedo when demodulating) and
//                          the packed guide (n.xyz | valid), (P.xyz | 0) into the work range; with no pass it is the finish too
//   k_denoise_pass         one pass of the 5 x 5 B3-spline stencil at step s, taps straight from memory: a block is 64 x 4 pixels,
//                          a wave 64 consecutive x of one row, so every tap of a wave is a contiguous row of float4 (steps 4 and up)
//   k_denoise_pass_tiled   the same pass for s = 1, 2 with the block's tile and its halo of 2 s pixels loaded into LDS once: the
//                          form both steps take, measured faster than the direct one by more than the spread of both
//
// The last pass multiplies the albedo back in and writes the RGBA8 pixel through store_rgba8 (raygen_device.h), the function
// rdx_accumulate uses.  A pixel's result is a function of the order of its taps alone (dy outer, dx inner), which denoise_pixel
// fixes for both forms: every decomposition gives the same bits.  No transcendental is evaluated, every operation is rounded on
// its own (-ffp-contract=off), so the numpy restatement of tests/denoise_cases.py has equal bits.  A translation unit of its own,
// so that the code objects of the other units stay the ones they were (profiles/denoise_kernels.txt).
#include "kernels.h"

#include "denoise.h"
#include "raygen_device.h"

namespace rdx {

constexpr uint32_t DENOISE_BX = 64, DENOISE_BY = 4, DENOISE_BLOCK = DENOISE_BX * DENOISE_BY;
constexpr float DENOISE_MIN_ALBEDO = 0.015625f;

struct PassArgs {
    uint32_t W, H, step, squarings, flags;
    float sp, sc;               // sigma_position * (float)step, sigma_colour * 2^-j: one rounded product each, taken on the host
};

__device__ __forceinline__ bool denoise_valid(const float4& guideN) { return __float_as_uint(guideN.w) == 1u; }
__device__ __forceinline__ float denoise_lum(const float4& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }
__device__ __forceinline__ bool denoise_finite(float v) { return fabsf(v) < __builtin_inff(); }      // false for a NaN

// den of the specification; fmaxf drops a NaN albedo
__device__ __forceinline__ f3 denoise_den(const float4& albedo, uint32_t flags)
{
    if (!(flags & DENOISE_DEMODULATE)) return mk3(1.0f, 1.0f, 1.0f);
    return mk3(cl_max(albedo.x, DENOISE_MIN_ALBEDO), cl_max(albedo.y, DENOISE_MIN_ALBEDO), cl_max(albedo.z, DENOISE_MIN_ALBEDO));
}

// out[p] and image[p] of the last iterate `it` (whose w carries the colour's): an invalid pixel's iterate is its colour's bits
__device__ __forceinline__ void denoise_finish(float4 it, bool valid, const float4* __restrict__ materials, uint32_t p, uint32_t flags,
                                               float4* __restrict__ out, uchar4* __restrict__ image)
{
    if (valid && (flags & DENOISE_DEMODULATE)) {
        const f3 den = denoise_den(materials[4 * (size_t)p + 1], flags);
        it.x = it.x * den.x; it.y = it.y * den.y; it.z = it.z * den.z;
    }
    out[p] = it;
    if (image) store_rgba8(image + p, mk3(it.x, it.y, it.z), (flags & DENOISE_DEBUG) ? 1u : 0u);
}

// i_{j+1}(p) of pixel (x, y): tap(qx, qy, nq, Pq, iq) fetches guide and iterate of a pixel inside the image
template <class Tap>
__device__ __forceinline__ float4 denoise_pixel(const PassArgs& a, int x, int y, const float4& ip, const float4& np, const float4& Pp, Tap&& tap)
{
    if (!denoise_valid(np)) return ip;
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const f3 n = mk3(np.x, np.y, np.z), P = mk3(Pp.x, Pp.y, Pp.z);
    const float lp = denoise_lum(ip);
    const int s = (int)a.step;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s, qy = y + dy * s;
            if (qx < 0 || qx >= (int)a.W || qy < 0 || qy >= (int)a.H) continue;
            float4 nq, Pq, iq;
            tap(qx, qy, nq, Pq, iq);
            if (!denoise_valid(nq)) continue;
            const float k = h[dy + 2] * h[dx + 2];
            float t = cl_max(dot3(n, mk3(nq.x, nq.y, nq.z)), 0.0f);
            for (uint32_t r = 0; r < a.squarings; ++r) t = t * t;
            float wz = 1.0f, wc = 1.0f;
            if (a.flags & DENOISE_POSITION) wz = cl_max(1.0f - fabsf(dot3(n, mk3(Pq.x, Pq.y, Pq.z) - P)) / a.sp, 0.0f);
            if (a.flags & DENOISE_COLOUR) {
                const float d = fabsf(lp - denoise_lum(iq)) / a.sc;
                wc = 1.0f / (1.0f + d * d);
            }
            const float w = ((k * t) * wz) * wc;
            if (!(w > 0.0f) || !denoise_finite(iq.x) || !denoise_finite(iq.y) || !denoise_finite(iq.z)) continue;
            sx = sx + iq.x * w; sy = sy + iq.y * w; sz = sz + iq.z * w;
            sw = sw + w;
        }
    }
    if (!(sw > 0.0f)) return ip;
    return make_float4(sx / sw, sy / sw, sz / sw, ip.w);
}

__global__ void __launch_bounds__(DENOISE_BLOCK)
k_denoise_prepare(const float4* __restrict__ color, const float4* __restrict__ materials, const float4* __restrict__ surfaces, uint32_t n, uint32_t flags,
                  float4* __restrict__ iterate, float4* __restrict__ guideN, float4* __restrict__ guideP, uint32_t finish, float4* __restrict__ out,
                  uchar4* __restrict__ image)
{
    const uint32_t p = blockIdx.x * DENOISE_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float4 m0 = materials[4 * (size_t)p], s0 = surfaces[4 * (size_t)p];
    const bool valid = __float_as_uint(m0.w) == 1u && __float_as_uint(s0.w) == 1u;
    float4 c = color[p];
    if (valid) {
        const f3 den = denoise_den(materials[4 * (size_t)p + 1], flags);
        c.x = c.x / den.x; c.y = c.y / den.y; c.z = c.z / den.z;
    }
    if (finish) { denoise_finish(c, valid, materials, p, flags, out, image); return; }
    iterate[p] = c;
    guideN[p] = make_float4(m0.x, m0.y, m0.z, __uint_as_float(valid ? 1u : 0u));
    guideP[p] = make_float4(s0.x, s0.y, s0.z, 0.0f);
}

// finish != 0: the last pass; dst is the caller's `out`
__global__ void __launch_bounds__(DENOISE_BLOCK)
k_denoise_pass(const float4* __restrict__ src, const float4* __restrict__ guideN, const float4* __restrict__ guideP, float4* __restrict__ dst, PassArgs a,
               uint32_t finish, const float4* __restrict__ materials, uchar4* __restrict__ image)
{
    const uint32_t x = blockIdx.x * DENOISE_BX + (threadIdx.x & (DENOISE_BX - 1u)), y = blockIdx.y * DENOISE_BY + threadIdx.x / DENOISE_BX;
    if (x >= a.W || y >= a.H) return;
    const uint32_t p = y * a.W + x;
    const float4 np = guideN[p];
    const float4 r = denoise_pixel(a, (int)x, (int)y, src[p], np, guideP[p], [&](int qx, int qy, float4& nq, float4& Pq, float4& iq) {
        const uint32_t q = (uint32_t)qy * a.W + (uint32_t)qx;
        nq = guideN[q]; Pq = guideP[q]; iq = src[q];
    });
    if (finish) denoise_finish(r, denoise_valid(np), materials, p, a.flags, dst, image);
    else dst[p] = r;
}

// The pass at step S from an LDS tile of (64 + 4 S) x (4 + 4 S) pixels, three float4 planes: 26112 bytes for S = 1, 41472 for S = 2.
// A tile pixel outside the image is marked invalid and never read: denoise_pixel asks for pixels inside the image only.
template <uint32_t S>
__global__ void __launch_bounds__(DENOISE_BLOCK)
k_denoise_pass_tiled(const float4* __restrict__ src, const float4* __restrict__ guideN, const float4* __restrict__ guideP, float4* __restrict__ dst, PassArgs a,
                     uint32_t finish, const float4* __restrict__ materials, uchar4* __restrict__ image)
{
    constexpr uint32_t TW = DENOISE_BX + 4u * S, TH = DENOISE_BY + 4u * S;
    __shared__ float4 s_it[TW * TH], s_n[TW * TH], s_p[TW * TH];
    const int x0 = (int)(blockIdx.x * DENOISE_BX) - 2 * (int)S, y0 = (int)(blockIdx.y * DENOISE_BY) - 2 * (int)S;
    for (uint32_t t = threadIdx.x; t < TW * TH; t += DENOISE_BLOCK) {
        const int gx = x0 + (int)(t % TW), gy = y0 + (int)(t / TW);
        if (gx >= 0 && gx < (int)a.W && gy >= 0 && gy < (int)a.H) {
            const uint32_t q = (uint32_t)gy * a.W + (uint32_t)gx;
            s_it[t] = src[q]; s_n[t] = guideN[q]; s_p[t] = guideP[q];
        } else {
            s_n[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & (DENOISE_BX - 1u), ly = threadIdx.x / DENOISE_BX;
    const uint32_t x = blockIdx.x * DENOISE_BX + lx, y = blockIdx.y * DENOISE_BY + ly;
    if (x >= a.W || y >= a.H) return;
    const uint32_t p = y * a.W + x, c = (ly + 2u * S) * TW + lx + 2u * S;
    const float4 np = s_n[c];
    const float4 r = denoise_pixel(a, (int)x, (int)y, s_it[c], np, s_p[c], [&](int qx, int qy, float4& nq, float4& Pq, float4& iq) {
        const uint32_t t = (uint32_t)(qy - y0) * TW + (uint32_t)(qx - x0);
        nq = s_n[t]; Pq = s_p[t]; iq = s_it[t];
    });
    if (finish) denoise_finish(r, denoise_valid(np), materials, p, a.flags, dst, image);
    else dst[p] = r;
}

void launch_denoise(hipStream_t st, const DenoiseArgs& d, const float4* color, const float4* materials, const float4* surfaces, float4* work, float4* out,
                    uchar4* image)
{
    const uint32_t n = d.W * d.H;
    if (!n) return;
    float4* iterate = work;
    float4* guideN = work + n;
    float4* guideP = work + 2 * (size_t)n;
    // pass j reads `cur` and writes the other of {work's iterate, out}; the last one writes out: the first iterate goes to the
    // work range for an odd number of passes, to out for an even one
    float4* cur = (d.passes & 1u) ? iterate : out;
    hipLaunchKernelGGL(k_denoise_prepare, dim3((n + DENOISE_BLOCK - 1u) / DENOISE_BLOCK), dim3(DENOISE_BLOCK), 0, st, color, materials, surfaces, n, d.flags, cur,
                       guideN, guideP, d.passes ? 0u : 1u, out, image);
    const dim3 grid((d.W + DENOISE_BX - 1u) / DENOISE_BX, (d.H + DENOISE_BY - 1u) / DENOISE_BY);
    for (uint32_t j = 0; j < d.passes; ++j) {
        PassArgs a{d.W, d.H, 1u << j, d.squarings, d.flags & (DENOISE_DEMODULATE | DENOISE_DEBUG), 0.0f, 0.0f};
        if (d.sigmaPosition != 0.0f) { a.flags |= DENOISE_POSITION; a.sp = d.sigmaPosition * (float)a.step; }
        if (d.sigmaColour != 0.0f) { a.flags |= DENOISE_COLOUR; a.sc = d.sigmaColour * (1.0f / (float)a.step); }
        float4* next = cur == out ? iterate : out;
        const uint32_t finish = j + 1u == d.passes ? 1u : 0u;
        if (j == 0 && (d.tiled & 1u))
            hipLaunchKernelGGL(k_denoise_pass_tiled<1u>, grid, dim3(DENOISE_BLOCK), 0, st, cur, guideN, guideP, next, a, finish, materials, image);
        else if (j == 1 && (d.tiled & 2u))
            hipLaunchKernelGGL(k_denoise_pass_tiled<2u>, grid, dim3(DENOISE_BLOCK), 0, st, cur, guideN, guideP, next, a, finish, materials, image);
        else
            hipLaunchKernelGGL(k_denoise_pass, grid, dim3(DENOISE_BLOCK), 0, st, cur, guideN, guideP, next, a, finish, materials, image);
        cur = next;
    }
}

} // namespace rdx

// svgf.hip -- device side of rdx_svgf_filter (include/rdx.h): the a-trous filter of rdx_denoise with SVGF's luminance
// weight, normalised by the local standard deviation of the variance rdx_temporal_accumulate estimates, and with that variance
// filtered along by the squared weights --
//
//   k_svgf_prepare      one pixel per lane: the first iterate (the colour, divided by the clamped albedo when demodulating | the
//                       variance, divided by the squared luminance of that albedo) and the packed guide (n.xyz | valid), (P.xyz | 0)
//                       into the work range; with no pass it is the finish too
//   k_svgf_pass         one pass at step s, the 3 x 3 prefilter of the variance and the 25 taps straight from memory: a block is
//                       64 x 4 pixels, a wave 64 consecutive x of one row, so every tap of a wave is a contiguous row of float4
//   k_svgf_pass_tiled   the same pass for s = 1, 2 with the block's tile and its halo of 2 s pixels in LDS; the halo holds the
//                       prefilter's neighbours at distance 1 as well
//
// The pass after which the caller asked for the feedback writes it beside its iterate; the last pass multiplies the albedo back in,
// writes `out`, the variance and the RGBA8 pixel through store_rgba8 (raygen_device.h).  A pixel's result is a function of the order
// of its taps alone, which svgf_pixel fixes for both forms.  No transcendental is evaluated, every operation is rounded on its own
// (-ffp-contract=off), the division and sqrtf are the correctly rounded ones, so the numpy restatement of tests/svgf_cases.py has
// equal bits.  The helpers denoise.hip has under other names are restated here: a translation unit of its own, so that the code
// objects of the other units stay the ones they were (profiles/svgf_kernels.txt).
#include "kernels.h"

#include "svgf.h"
#include "raygen_device.h"

namespace rdx {

constexpr uint32_t SVGF_BX = 64, SVGF_BY = 4, SVGF_BLOCK = SVGF_BX * SVGF_BY;
constexpr float SVGF_MIN_ALBEDO = 0.015625f;

struct SvgfPassArgs {
    uint32_t W, H, step, squarings, flags;
    float sp, sl, eps;          // sigma_position * (float)step (one rounded product, taken on the host), sigma_luminance, epsilon
};

// what the pass that ends the filter, or the one the feedback is taken after, writes beside its iterate; all but color may be null
struct SvgfEmit {
    const float4* color;
    const float4* materials;
    float4* out;
    float* variance;
    float4* feedback;
    uchar4* image;
};

__device__ __forceinline__ bool svgf_valid(const float4& guideN) { return __float_as_uint(guideN.w) == 1u; }
__device__ __forceinline__ float svgf_lum(float r, float g, float b) { return (0.2126f * r + 0.7152f * g) + 0.0722f * b; }
__device__ __forceinline__ bool svgf_finite(float v) { return fabsf(v) < __builtin_inff(); }      // false for a NaN

// den of the specification; fmaxf drops a NaN albedo
__device__ __forceinline__ f3 svgf_den(const float4& albedo, uint32_t flags)
{
    if (!(flags & DENOISE_DEMODULATE)) return mk3(1.0f, 1.0f, 1.0f);
    return mk3(cl_max(albedo.x, SVGF_MIN_ALBEDO), cl_max(albedo.y, SVGF_MIN_ALBEDO), cl_max(albedo.z, SVGF_MIN_ALBEDO));
}
// ld of the specification
__device__ __forceinline__ float svgf_ld(const f3& den, uint32_t flags) { return (flags & DENOISE_DEMODULATE) ? svgf_lum(den.x, den.y, den.z) : 1.0f; }

// feedback[p], out[p], variance_out[p] and image[p] of the iterate `it` (rgb | v): an invalid pixel's iterate is its colour's bits
__device__ __forceinline__ void svgf_emit(const SvgfEmit& e, float4 it, bool valid, uint32_t p, uint32_t flags)
{
    float v = 0.0f;
    if (valid) {
        const f3 den = svgf_den(e.materials[4 * (size_t)p + 1], flags);
        const float ld = svgf_ld(den, flags);
        it.x = it.x * den.x; it.y = it.y * den.y; it.z = it.z * den.z;
        v = it.w * (ld * ld);
    }
    it.w = e.color[p].w;
    if (e.feedback) e.feedback[p] = it;
    if (!e.out) return;
    e.out[p] = it;
    if (e.variance) e.variance[p] = v;
    if (e.image) store_rgba8(e.image + p, mk3(it.x, it.y, it.z), (flags & DENOISE_DEBUG) ? 1u : 0u);
}

// (i_{j+1} | v_{j+1})(p) of pixel (x, y).  var(qx, qy, vq) -> valid(q), and v_j(q) of a valid q; tap(qx, qy, nq, Pq, iq) fetches guide
// and iterate; both are asked for pixels inside the image only
template <class Var, class Tap>
__device__ __forceinline__ float4 svgf_pixel(const SvgfPassArgs& a, int x, int y, const float4& ip, const float4& np, const float4& Pp, Var&& var, Tap&& tap)
{
    if (!svgf_valid(np)) return ip;
    float dl = 0.0f;
    if (a.flags & SVGF_LUMINANCE) {
        constexpr float g[3] = {0.25f, 0.5f, 0.25f};
        float gs = 0.0f, gw = 0.0f;
#pragma unroll
        for (int dy = -1; dy <= 1; ++dy) {
#pragma unroll
            for (int dx = -1; dx <= 1; ++dx) {
                const int qx = x + dx, qy = y + dy;
                if (qx < 0 || qx >= (int)a.W || qy < 0 || qy >= (int)a.H) continue;
                float vq;
                if (!var(qx, qy, vq)) continue;
                const float k = g[dy + 1] * g[dx + 1];
                gs = gs + k * vq;
                gw = gw + k;
            }
        }
        dl = a.sl * sqrtf(gs / gw) + a.eps;
    }
    constexpr float h[5] = {0.0625f, 0.25f, 0.375f, 0.25f, 0.0625f};
    const f3 n = mk3(np.x, np.y, np.z), P = mk3(Pp.x, Pp.y, Pp.z);
    const float lp = svgf_lum(ip.x, ip.y, ip.z);
    const int s = (int)a.step;
    float sx = 0.0f, sy = 0.0f, sz = 0.0f, sv = 0.0f, sw = 0.0f;
#pragma unroll
    for (int dy = -2; dy <= 2; ++dy) {
#pragma unroll
        for (int dx = -2; dx <= 2; ++dx) {
            const int qx = x + dx * s, qy = y + dy * s;
            if (qx < 0 || qx >= (int)a.W || qy < 0 || qy >= (int)a.H) continue;
            float4 nq, Pq, iq;
            tap(qx, qy, nq, Pq, iq);
            if (!svgf_valid(nq)) continue;
            const float k = h[dy + 2] * h[dx + 2];
            float t = cl_max(dot3(n, mk3(nq.x, nq.y, nq.z)), 0.0f);
            for (uint32_t r = 0; r < a.squarings; ++r) t = t * t;
            float wz = 1.0f, wc = 1.0f;
            if (a.flags & DENOISE_POSITION) wz = cl_max(1.0f - fabsf(dot3(n, mk3(Pq.x, Pq.y, Pq.z) - P)) / a.sp, 0.0f);
            if (a.flags & SVGF_LUMINANCE) {
                const float d = fabsf(lp - svgf_lum(iq.x, iq.y, iq.z)) / dl;
                wc = 1.0f / (1.0f + d * d);
            }
            const float w = ((k * t) * wz) * wc;
            if (!(w > 0.0f) || !svgf_finite(iq.x) || !svgf_finite(iq.y) || !svgf_finite(iq.z) || !svgf_finite(iq.w)) continue;
            sx = sx + iq.x * w; sy = sy + iq.y * w; sz = sz + iq.z * w;
            sv = sv + iq.w * (w * w);
            sw = sw + w;
        }
    }
    if (!(sw > 0.0f)) return ip;
    return make_float4(sx / sw, sy / sw, sz / sw, sv / (sw * sw));
}

__global__ void __launch_bounds__(SVGF_BLOCK)
k_svgf_prepare(const float4* __restrict__ moments, const float4* __restrict__ surfaces, uint32_t n, uint32_t flags, float4* __restrict__ iterate,
               float4* __restrict__ guideN, float4* __restrict__ guideP, uint32_t finish, SvgfEmit e)
{
    const uint32_t p = blockIdx.x * SVGF_BLOCK + threadIdx.x;
    if (p >= n) return;
    const float4 m0 = e.materials[4 * (size_t)p], s0 = surfaces[4 * (size_t)p];
    const bool valid = __float_as_uint(m0.w) == 1u && __float_as_uint(s0.w) == 1u;
    float4 c = e.color[p];
    c.w = 0.0f;
    if (valid) {
        const f3 den = svgf_den(e.materials[4 * (size_t)p + 1], flags);
        const float ld = svgf_ld(den, flags), vz = moments[p].z;
        c.x = c.x / den.x; c.y = c.y / den.y; c.z = c.z / den.z;
        if (vz > 0.0f && vz < __builtin_inff()) c.w = vz / (ld * ld);
    }
    if (finish) { svgf_emit(e, c, valid, p, flags); return; }
    iterate[p] = c;
    guideN[p] = make_float4(m0.x, m0.y, m0.z, __uint_as_float(valid ? 1u : 0u));
    guideP[p] = make_float4(s0.x, s0.y, s0.z, 0.0f);
}

// dst: the next iterate, null for the last pass, which writes e.out instead; e.feedback is set for one pass at the most
__global__ void __launch_bounds__(SVGF_BLOCK)
k_svgf_pass(const float4* __restrict__ src, const float4* __restrict__ guideN, const float4* __restrict__ guideP, float4* __restrict__ dst, SvgfPassArgs a, SvgfEmit e)
{
    const uint32_t x = blockIdx.x * SVGF_BX + (threadIdx.x & (SVGF_BX - 1u)), y = blockIdx.y * SVGF_BY + threadIdx.x / SVGF_BX;
    if (x >= a.W || y >= a.H) return;
    const uint32_t p = y * a.W + x;
    const float4 np = guideN[p];
    const float4 r = svgf_pixel(a, (int)x, (int)y, src[p], np, guideP[p],
        [&](int qx, int qy, float& vq) {
            const uint32_t q = (uint32_t)qy * a.W + (uint32_t)qx;
            if (__float_as_uint(guideN[q].w) != 1u) return false;
            vq = src[q].w;
            return true;
        },
        [&](int qx, int qy, float4& nq, float4& Pq, float4& iq) {
            const uint32_t q = (uint32_t)qy * a.W + (uint32_t)qx;
            nq = guideN[q]; Pq = guideP[q]; iq = src[q];
        });
    if (dst) dst[p] = r;
    if (e.out || e.feedback) svgf_emit(e, r, svgf_valid(np), p, a.flags);
}

// The pass at step S from an LDS tile of (64 + 4 S) x (4 + 4 S) pixels, three float4 planes: 26112 bytes for S = 1, 41472 for S = 2.
// A tile pixel outside the image is marked invalid and never read: svgf_pixel asks for pixels inside the image only, and those it
// asks for lie within 2 S >= 1 of the block.
template <uint32_t S>
__global__ void __launch_bounds__(SVGF_BLOCK)
k_svgf_pass_tiled(const float4* __restrict__ src, const float4* __restrict__ guideN, const float4* __restrict__ guideP, float4* __restrict__ dst, SvgfPassArgs a,
                  SvgfEmit e)
{
    constexpr uint32_t TW = SVGF_BX + 4u * S, TH = SVGF_BY + 4u * S;
    __shared__ float4 s_it[TW * TH], s_n[TW * TH], s_p[TW * TH];
    const int x0 = (int)(blockIdx.x * SVGF_BX) - 2 * (int)S, y0 = (int)(blockIdx.y * SVGF_BY) - 2 * (int)S;
    for (uint32_t t = threadIdx.x; t < TW * TH; t += SVGF_BLOCK) {
        const int gx = x0 + (int)(t % TW), gy = y0 + (int)(t / TW);
        if (gx >= 0 && gx < (int)a.W && gy >= 0 && gy < (int)a.H) {
            const uint32_t q = (uint32_t)gy * a.W + (uint32_t)gx;
            s_it[t] = src[q]; s_n[t] = guideN[q]; s_p[t] = guideP[q];
        } else {
            s_n[t] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        }
    }
    __syncthreads();
    const uint32_t lx = threadIdx.x & (SVGF_BX - 1u), ly = threadIdx.x / SVGF_BX;
    const uint32_t x = blockIdx.x * SVGF_BX + lx, y = blockIdx.y * SVGF_BY + ly;
    if (x >= a.W || y >= a.H) return;
    const uint32_t p = y * a.W + x, c = (ly + 2u * S) * TW + lx + 2u * S;
    const float4 np = s_n[c];
    const float4 r = svgf_pixel(a, (int)x, (int)y, s_it[c], np, s_p[c],
        [&](int qx, int qy, float& vq) {
            const uint32_t t = (uint32_t)(qy - y0) * TW + (uint32_t)(qx - x0);
            if (__float_as_uint(s_n[t].w) != 1u) return false;
            vq = s_it[t].w;
            return true;
        },
        [&](int qx, int qy, float4& nq, float4& Pq, float4& iq) {
            const uint32_t t = (uint32_t)(qy - y0) * TW + (uint32_t)(qx - x0);
            nq = s_n[t]; Pq = s_p[t]; iq = s_it[t];
        });
    if (dst) dst[p] = r;
    if (e.out || e.feedback) svgf_emit(e, r, svgf_valid(np), p, a.flags);
}

void launch_svgf_filter(hipStream_t st, const SvgfArgs& d, const float4* color, const float4* moments, const float4* materials, const float4* surfaces,
                        float4* work, float4* out, float* variance_out, float4* feedback, uchar4* image)
{
    const uint32_t n = d.W * d.H;
    if (!n) return;
    float4* iterate = work;
    float4* guideN = work + n;
    float4* guideP = work + 2 * (size_t)n;
    const uint32_t base = d.flags & (DENOISE_DEMODULATE | DENOISE_DEBUG);
    const SvgfEmit last{color, materials, out, variance_out, d.feedbackPass == d.passes ? feedback : nullptr, image};
    // pass j reads `cur` and writes the other of {work's iterate, out}; the last one writes out in its final form: the first iterate
    // goes to the work range for an odd number of passes, to out for an even one
    float4* cur = (d.passes & 1u) ? iterate : out;
    hipLaunchKernelGGL(k_svgf_prepare, dim3((n + SVGF_BLOCK - 1u) / SVGF_BLOCK), dim3(SVGF_BLOCK), 0, st, moments, surfaces, n, base, cur, guideN, guideP,
                       d.passes ? 0u : 1u, d.passes ? SvgfEmit{color, materials, nullptr, nullptr, nullptr, nullptr} : last);
    const dim3 grid((d.W + SVGF_BX - 1u) / SVGF_BX, (d.H + SVGF_BY - 1u) / SVGF_BY);
    for (uint32_t j = 0; j < d.passes; ++j) {
        SvgfPassArgs a{d.W, d.H, 1u << j, d.squarings, base, 0.0f, d.sigmaLuminance, d.epsilon};
        if (d.sigmaPosition != 0.0f) { a.flags |= DENOISE_POSITION; a.sp = d.sigmaPosition * (float)a.step; }
        if (d.sigmaLuminance != 0.0f) a.flags |= SVGF_LUMINANCE;
        const bool finish = j + 1u == d.passes;
        float4* next = cur == out ? iterate : out;
        float4* dst = finish ? nullptr : next;
        const SvgfEmit e = finish ? last : SvgfEmit{color, materials, nullptr, nullptr, j + 1u == d.feedbackPass ? feedback : nullptr, nullptr};
        if (j == 0 && (d.tiled & 1u))
            hipLaunchKernelGGL(k_svgf_pass_tiled<1u>, grid, dim3(SVGF_BLOCK), 0, st, cur, guideN, guideP, dst, a, e);
        else if (j == 1 && (d.tiled & 2u))
            hipLaunchKernelGGL(k_svgf_pass_tiled<2u>, grid, dim3(SVGF_BLOCK), 0, st, cur, guideN, guideP, dst, a, e);
        else
            hipLaunchKernelGGL(k_svgf_pass, grid, dim3(SVGF_BLOCK), 0, st, cur, guideN, guideP, dst, a, e);
        cur = next;
    }
}

} // namespace rdx

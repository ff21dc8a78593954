// temporal.hip -- device side of rdx_camera_view and rdx_temporal_accumulate (include/rdx.h): the temporal half of SVGF
// over a frame of float4 colours, guided by the primary hits' material and surface records --
//
//   k_camera_view          one thread: the 64-byte view record (eye | right | up | back, with width, height, kx, ky in the w's) of the
//                          camera buffer's current contents, from the matrices and the OCML cos / sin of k_raygen_camera (raygen.hip)
//   k_temporal_reproject   one pixel per lane: the pixel's motion through the two views, the four bilinear taps of the history that
//                          pass the consistency tests, the exponential means of colour and luminance moments, the temporal variance,
//                          all four planes of the new history and the RGBA8 pixel through store_rgba8 (raygen_device.h)
//   k_temporal_variance    one pixel per lane, after the first kernel has written every pixel: the 7 x 7 spatial estimate of the
//                          variance from the new moments for pixels younger than variance_min_history; every other lane leaves at once
//
// A block is 64 x 4 pixels, a wave 64 consecutive x of one row: a tap of a wave is a contiguous row of float4 per plane.  Every
// address is a pixel index below W H of a range the host has checked; a tap's coordinates pass the inside-the-image test before an
// address is formed.  No transcendental is evaluated per pixel, every operation is rounded on its own (-ffp-contract=off), so the
// numpy restatement of tests/temporal_cases.py has equal bits.  A translation unit of its own, so that the code objects of the other
// units stay the ones they were (profiles/temporal_kernels.txt).
#include "kernels.h"

#include "temporal.h"
#include "raygen_device.h"

namespace rdx {

constexpr uint32_t TEMPORAL_BX = 64, TEMPORAL_BY = 4, TEMPORAL_BLOCK = TEMPORAL_BX * TEMPORAL_BY;

struct ViewArgs { f3 eye, right, up, back; float width, height, kx, ky; };

__device__ __forceinline__ ViewArgs load_view(const float4* __restrict__ v)
{
    const float4 a = v[0], b = v[1], c = v[2], d = v[3];
    return ViewArgs{mk3(a.x, a.y, a.z), mk3(b.x, b.y, b.z), mk3(c.x, c.y, c.z), mk3(d.x, d.y, d.z), a.w, b.w, c.w, d.w};
}
__device__ __forceinline__ float temporal_lum(const f3& c) { return (0.2126f * c.x + 0.7152f * c.y) + 0.0722f * c.z; }      // denoise_lum's order
__device__ __forceinline__ bool temporal_finite(float v) { return fabsf(v) < __builtin_inff(); }      // false for a NaN
__device__ __forceinline__ bool temporal_finite3(const f3& c) { return temporal_finite(c.x) && temporal_finite(c.y) && temporal_finite(c.z); }

// (u, t): the sample-space position of the world point Q under V -- the inverse of camera_ray for fStop == 0; false: Q is not in
// front of the camera
__device__ __forceinline__ bool temporal_project(const ViewArgs& V, f3 Q, float& u, float& t)
{
    const f3 v = Q - V.eye;
    const float dz = -dot3(V.back, v);
    u = V.width * 0.5f + (V.width * V.kx) * (dot3(V.right, v) / dz);
    t = V.height * 0.5f - (V.height * V.ky) * (dot3(V.up, v) / dz);
    return dz > 0.0f;
}

// c = (a b) of two row-major 3 x 3 matrices, every element (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j
__device__ __forceinline__ void mat3_mul(const float* a, const float* b, float* c)
{
#pragma unroll
    for (int i = 0; i < 3; ++i)
#pragma unroll
        for (int j = 0; j < 3; ++j) c[3 * i + j] = (a[3 * i] * b[j] + a[3 * i + 1] * b[3 + j]) + a[3 * i + 2] * b[6 + j];
}

__global__ void k_camera_view(const PhysicalCamera* __restrict__ camera, float4* __restrict__ view)
{
    const PhysicalCamera cam = *camera;
    const float cx = cosf(cam.wx), sx = sinf(cam.wx), cy = cosf(cam.wy), sy = sinf(cam.wy), cz = cosf(cam.wz), sz = sinf(cam.wz);
    const float rx[9] = {1, 0, 0, 0, cx, -sx, 0, sx, cx};
    const float ry[9] = {cy, 0, sy, 0, 1, 0, -sy, 0, cy};
    const float rz[9] = {cz, -sz, 0, sz, cz, 0, 0, 0, 1};
    float t[9], m[9];
    mat3_mul(ry, rz, t);
    mat3_mul(rx, t, m);
    const float kx = cam.focalLength / cam.sensorWidth;
    const float ky = cam.focalLength / (cam.sensorWidth * (cam.heightPixel / cam.widthPixel));
    view[0] = make_float4(cam.x, cam.y, cam.z, cam.widthPixel);
    view[1] = make_float4(m[0], m[3], m[6], cam.heightPixel);
    view[2] = make_float4(m[1], m[4], m[7], kx);
    view[3] = make_float4(m[2], m[5], m[8], ky);
}

__global__ void __launch_bounds__(TEMPORAL_BLOCK)
k_temporal_reproject(const float4* __restrict__ color, const float4* __restrict__ materials, const float4* __restrict__ surfaces,
                     const float4* __restrict__ previousPositions, const float4* __restrict__ view, const float4* __restrict__ previousView,
                     const float4* __restrict__ historyIn, float4* __restrict__ historyOut, uchar4* __restrict__ image, TemporalArgs a)
{
    const uint32_t x = blockIdx.x * TEMPORAL_BX + (threadIdx.x & (TEMPORAL_BX - 1u)), y = blockIdx.y * TEMPORAL_BY + threadIdx.x / TEMPORAL_BX;
    if (x >= a.W || y >= a.H) return;
    const size_t n = (size_t)a.W * a.H;
    const uint32_t p = y * a.W + x;
    const float4 m0 = materials[4 * (size_t)p], m1r = materials[4 * (size_t)p + 1], s0 = surfaces[4 * (size_t)p];
    const float4 c4 = color[p];
    const f3 c = mk3(c4.x, c4.y, c4.z), nrm = mk3(m0.x, m0.y, m0.z), P = mk3(s0.x, s0.y, s0.z);
    const uint32_t mi = __float_as_uint(m1r.w);
    const bool valid = __float_as_uint(m0.w) == 1u && __float_as_uint(s0.w) == 1u;
    historyOut[2 * n + p] = make_float4(nrm.x, nrm.y, nrm.z, m1r.w);
    historyOut[3 * n + p] = make_float4(P.x, P.y, P.z, __uint_as_float(valid ? 1u : 0u));
    const uint32_t debug = (a.flags & TEMPORAL_DEBUG) ? 1u : 0u;
    if (!valid) {
        historyOut[p] = c4;
        historyOut[n + p] = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
        if (image) store_rgba8(image + p, c, debug);
        return;
    }

    float sw = 0.0f, sx = 0.0f, sy = 0.0f, sz = 0.0f, s1 = 0.0f, s2 = 0.0f;
    uint32_t Nh = 0xffffffffu;
    if (historyIn) {
        f3 Q = P;
        if (previousPositions) { const float4 q4 = previousPositions[p]; Q = mk3(q4.x, q4.y, q4.z); }
        float uc, tc, up, tp;
        const bool frontC = temporal_project(load_view(view), P, uc, tc);
        const bool frontP = temporal_project(load_view(previousView), Q, up, tp);
        const float du = up - uc, dt = tp - tc;
        if (frontC && frontP && temporal_finite(du) && temporal_finite(dt)) {
            const float hx = (float)x + du, hy = (float)y + dt;
            const float x0f = floorf(hx), y0f = floorf(hy);
            const float fx = hx - x0f, fy = hy - y0f;
            // outside -1 .. W (-1 .. H) every tap is outside the image; inside, the conversion to int is exact
            if (x0f >= -1.0f && x0f <= (float)a.W && y0f >= -1.0f && y0f <= (float)a.H) {
                const int x0 = (int)x0f, y0 = (int)y0f;
                const float wx[2] = {1.0f - fx, fx}, wy[2] = {1.0f - fy, fy};
#pragma unroll
                for (int j = 0; j < 2; ++j) {
#pragma unroll
                    for (int i = 0; i < 2; ++i) {
                        const int qx = x0 + i, qy = y0 + j;
                        if (qx < 0 || qx >= (int)a.W || qy < 0 || qy >= (int)a.H) continue;
                        const uint32_t q = (uint32_t)qy * a.W + (uint32_t)qx;
                        const float w = wx[i] * wy[j];
                        const float4 t1 = historyIn[n + q], t3 = historyIn[3 * n + q];
                        const uint32_t Nq = __float_as_uint(t1.w);
                        if (__float_as_uint(t3.w) != 1u || Nq < 1u) continue;
                        const float4 t2 = historyIn[2 * n + q];
                        if (__float_as_uint(t2.w) != mi) continue;
                        if (!(dot3(nrm, mk3(t2.x, t2.y, t2.z)) >= a.normalCosMin)) continue;
                        if ((a.flags & TEMPORAL_POSITION) && !(fabsf(dot3(nrm, mk3(t3.x, t3.y, t3.z) - Q)) <= a.positionTolerance)) continue;
                        const float4 t0 = historyIn[q];
                        if (!(w > 0.0f) || !temporal_finite3(mk3(t0.x, t0.y, t0.z))) continue;
                        sx = sx + t0.x * w; sy = sy + t0.y * w; sz = sz + t0.z * w;
                        s1 = s1 + t1.x * w; s2 = s2 + t1.y * w;
                        sw = sw + w;
                        Nh = Nq < Nh ? Nq : Nh;
                    }
                }
            }
        }
    }

    const bool fin = temporal_finite3(c);
    const float l = temporal_lum(c);
    uint32_t N;
    f3 co;
    float m1, m2;
    if (sw > 0.0f) {
        const f3 h = mk3(sx / sw, sy / sw, sz / sw);
        const float m1h = s1 / sw, m2h = s2 / sw;
        if (fin) {
            N = Nh >= a.maxHistory ? a.maxHistory : Nh + 1u;
            const float al = cl_max(1.0f / (float)N, a.alphaMin), am = cl_max(1.0f / (float)N, a.alphaMomentsMin);
            co = mk3(h.x + (c.x - h.x) * al, h.y + (c.y - h.y) * al, h.z + (c.z - h.z) * al);
            m1 = m1h + (l - m1h) * am;
            m2 = m2h + (l * l - m2h) * am;
        } else {            // a colour that is not finite keeps the history as it is
            N = Nh; co = h; m1 = m1h; m2 = m2h;
        }
    } else if (fin) {
        N = 1u; co = c; m1 = l; m2 = l * l;
    } else {                // nothing to keep: the colour passes through and is no one's tap
        N = 0u; co = c; m1 = 0.0f; m2 = 0.0f;
    }
    // the temporal variance; k_temporal_variance replaces it where N < variance_min_history
    const float var = cl_max(m2 - m1 * m1, 0.0f);
    historyOut[p] = make_float4(co.x, co.y, co.z, c4.w);
    historyOut[n + p] = make_float4(m1, m2, var, __uint_as_float(N));
    if (image) store_rgba8(image + p, co, debug);
}

// Plane 1's variance of the pixels younger than variance_min_history, from the moments the first kernel wrote: x, y and w of
// plane 1 are read here and only z is written, with a 4-byte store, so no lane reads what another one writes
__global__ void __launch_bounds__(TEMPORAL_BLOCK)
k_temporal_variance(float4* __restrict__ historyOut, TemporalArgs a)
{
    const uint32_t x = blockIdx.x * TEMPORAL_BX + (threadIdx.x & (TEMPORAL_BX - 1u)), y = blockIdx.y * TEMPORAL_BY + threadIdx.x / TEMPORAL_BX;
    if (x >= a.W || y >= a.H) return;
    const size_t n = (size_t)a.W * a.H;
    const uint32_t p = y * a.W + x;
    const float4 p1 = historyOut[n + p];
    const uint32_t N = __float_as_uint(p1.w);
    if (N >= a.varianceMinHistory) return;
    if (__float_as_uint(historyOut[3 * n + p].w) != 1u) return;
    const float4 p2 = historyOut[2 * n + p];
    const f3 nrm = mk3(p2.x, p2.y, p2.z);
    const uint32_t mi = __float_as_uint(p2.w);
    float sw = 0.0f, s1 = 0.0f, s2 = 0.0f;
    for (int dy = -3; dy <= 3; ++dy) {
        const int qy = (int)y + dy;
        if (qy < 0 || qy >= (int)a.H) continue;
#pragma unroll
        for (int dx = -3; dx <= 3; ++dx) {
            const int qx = (int)x + dx;
            if (qx < 0 || qx >= (int)a.W) continue;
            const uint32_t q = (uint32_t)qy * a.W + (uint32_t)qx;
            const float4 q1 = historyOut[n + q];
            if (__float_as_uint(q1.w) < 1u) continue;           // N >= 1: a valid pixel with moments (an invalid one has N = 0)
            const float4 q2 = historyOut[2 * n + q];
            if (__float_as_uint(q2.w) != mi) continue;
            const float w = cl_max(dot3(nrm, mk3(q2.x, q2.y, q2.z)), 0.0f);
            if (!(w > 0.0f) || !temporal_finite(w) || !temporal_finite(q1.x) || !temporal_finite(q1.y)) continue;
            s1 = s1 + q1.x * w; s2 = s2 + q1.y * w;
            sw = sw + w;
        }
    }
    const bool any = sw > 0.0f;
    const float M1 = any ? s1 / sw : p1.x, M2 = any ? s2 / sw : p1.y;
    const float boost = (float)a.varianceMinHistory / (float)(N > 1u ? N : 1u);
    reinterpret_cast<float*>(historyOut + n + p)[2] = cl_max(M2 - M1 * M1, 0.0f) * boost;
}

void launch_camera_view(hipStream_t st, const PhysicalCamera* camera, float4* view)
{
    hipLaunchKernelGGL(k_camera_view, dim3(1), dim3(1), 0, st, camera, view);
}

void launch_temporal_accumulate(hipStream_t st, const TemporalArgs& a, const float4* color, const float4* materials, const float4* surfaces,
                                const float4* previousPositions, const float4* view, const float4* previousView, const float4* historyIn, float4* historyOut,
                                uchar4* image)
{
    if (!a.W || !a.H) return;
    const dim3 grid((a.W + TEMPORAL_BX - 1u) / TEMPORAL_BX, (a.H + TEMPORAL_BY - 1u) / TEMPORAL_BY);
    hipLaunchKernelGGL(k_temporal_reproject, grid, dim3(TEMPORAL_BLOCK), 0, st, color, materials, surfaces, previousPositions, view, previousView, historyIn,
                       historyOut, image, a);
    if (a.varianceMinHistory)
        hipLaunchKernelGGL(k_temporal_variance, grid, dim3(TEMPORAL_BLOCK), 0, st, historyOut, a);
}

} // namespace rdx

// light_emit.h -- what one light gives at one shaded point, written ONCE for the per-hit calls (rdx_light_hits,
// rdx_punctual_light_hits, rdx_area_light_hits, rdx_env_light_hits) and the per-path calls (path_shade.h), so a path call has the bits of the per-hit
// calls by construction: one emit function per kind of light -- (L, E, tmax) seen from `above`, or dark --, one record function
// from that to the lit colour and the shadow ray, and the body of the three per-hit kernels.  Device code only.
//
// The PBR and frame functions are those of stages.h, called as `material` calls them.  The units that include this header are
// compiled with -ffp-contract=off: every float32 operation is rounded on its own, and d2, the cone's cosine, p, n and g are plain
// products and sums, NOT dot3 / cross3, which may fuse: numpy float32 restates them (tests/punctual_cases.py `emitted`,
// tests/area_cases.py `emitted_area`, tests/env_cases.py `sampled_env`).
#pragma once
#include "kernels.h"

#include "area.h"
#include "device_math.h"
#include "env.h"
#include "stages.h"

namespace rdx {

constexpr uint32_t LIGHT_HITS_BLOCK = 256;

// ---- emit: L = the unit direction towards the light, E = what it emits at `above`, tmax = the end of the shadow ray's interval;
// false: the record is dark there.  `lt` is the same address in every lane, so its fields arrive through the scalar cache and the
// branches on `type` and `flags` are uniform; the ones on d2, range, the cone and the geometry term are per lane. ----

// a DirLight of the scene: never dark, the stock interval (stages.h:276-278, 309-312 with this light in the place of lights[0])
__device__ __forceinline__ bool dir_emit(const DirLight* __restrict__ lt, f3& L, f3& E, float& tmax)
{
    L = normalize3(mk3(-lt->direction[0], -lt->direction[1], -lt->direction[2]));
    E = mk3(lt->color[0], lt->color[1], lt->color[2]);
    tmax = 1000.0f;
    return true;
}

// a record of a caller's punctual table (include/rdx.h rdx_punctual_light): type 0 is dir_emit; a point or spot light ends the
// shadow ray at its position
__device__ __forceinline__ bool punctual_emit(const PunctualLight* __restrict__ lt, const f3& above, f3& L, f3& E, float& tmax)
{
    const uint32_t type = lt->type;
    if (type > LIGHT_SPOT) return false;
    E = mk3(lt->color[0], lt->color[1], lt->color[2]);
    if (type == LIGHT_DIRECTIONAL) {
        L = normalize3(mk3(-lt->direction[0], -lt->direction[1], -lt->direction[2]));
        tmax = 1000.0f;
        return true;
    }
    const f3 v = mk3(lt->position[0] - above.x, lt->position[1] - above.y, lt->position[2] - above.z);
    const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    if (!(d2 > 0.0f)) return false;
    if (!(d2 < __builtin_inff())) return false;
    const float range = lt->range;
    if (range > 0.0f && !(d2 < range * range)) return false;
    L = normalize3(v);
    const float att = 1.0f / d2;
    E = E * att;
    tmax = sqrtf(d2);
    if (type == LIGHT_SPOT) {
        const f3 S = normalize3(mk3(lt->direction[0], lt->direction[1], lt->direction[2]));
        const float c = -((S.x * L.x + S.y * L.y) + S.z * L.z);
        const float f = cl_clamp(c * lt->coneScale + lt->coneOffset, 0.0f, 1.0f);
        if (!(f > 0.0f)) return false;
        E = E * (f * f);
    }
    return true;
}

// a record of a caller's area table (include/rdx.h rdx_area_light) with the random pair (u, v): the point p = corner + u edgeU + v
// edgeV of the emitter (the pair folded into the triangle for type 1), E = radiance x (emitter area x cosine at the emitter) /
// distance^2 -- the one-sample estimator under the pdf 1 / area --, tmax = 0.999 of the distance: the shadow ray stops short of the
// emitter.  Dark: unknown type, d2 zero or not finite, back face of a one-sided record, degenerate emitter, NaN.  n = cross(edgeU,
// edgeV) is NOT normalised: |n| is the parallelogram's area, so g = -dot(n, L) is area x cosine and no square root is taken.
__device__ __forceinline__ bool area_emit(const AreaLight* __restrict__ lt, const f3& above, float u, float v, f3& L, f3& E, float& tmax)
{
    const uint32_t type = lt->type;
    if (type > AREA_TRIANGLE) return false;
    if (type == AREA_TRIANGLE && u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
    const f3 eu = mk3(lt->edgeU[0], lt->edgeU[1], lt->edgeU[2]), ev = mk3(lt->edgeV[0], lt->edgeV[1], lt->edgeV[2]);
    const f3 p = mk3((lt->corner[0] + eu.x * u) + ev.x * v, (lt->corner[1] + eu.y * u) + ev.y * v, (lt->corner[2] + eu.z * u) + ev.z * v);
    const f3 n = mk3(eu.y * ev.z - eu.z * ev.y, eu.z * ev.x - eu.x * ev.z, eu.x * ev.y - eu.y * ev.x);
    const f3 w = mk3(p.x - above.x, p.y - above.y, p.z - above.z);
    const float d2 = (w.x * w.x + w.y * w.y) + w.z * w.z;
    if (!(d2 > 0.0f)) return false;
    if (!(d2 < __builtin_inff())) return false;
    L = normalize3(w);
    float g = -((n.x * L.x + n.y * L.y) + n.z * L.z);
    if (type == AREA_TRIANGLE) g = g * 0.5f;
    if (lt->flags & AREA_TWO_SIDED) g = fabsf(g);
    if (!(g > 0.0f)) return false;
    const float s = g / d2;
    E = mk3(lt->radiance[0] * s, lt->radiance[1] * s, lt->radiance[2] * s);
    tmax = sqrtf(d2) * 0.999f;
    return true;
}

// the random pair of area record `stream` on a path's key: paths are at most 62 deep, so no such third word is the bare depth
// rdx_scatter_hits draws from, or another stream's
__device__ __forceinline__ f3 area_random(uint32_t frameID, uint32_t pixel, uint32_t depth, uint32_t stream)
{
    return pcg3d(frameID, pixel, depth + ((stream + 1u) << 16));
}

// the environment (include/rdx.h rdx_env_light_hits; env.h for the table) with the random triple (u, v, z): u chooses the row y in
// M and the place fy inside its band of cos(theta), v the column x in row y of C, z the place fx inside the texel.  E = texel x
// (total / q) x the texel's solid angle -- the one-sample estimator under the pdf q / (total x solid angle) --, the interval is the
// stock one, as for a directional light.  Dark: no light in the image (total 0), a header that is not the call's, q == 0.  `env` is
// the same in every lane, so the header arrives through the scalar cache; the searches are per lane.  Both are bounded by the CALL's
// H and W and every index stays inside [0, H) / [0, W): a table of garbage gives unspecified colours, never a read outside the
// image or the table.  u can be exactly 1.0 (pcg3d divides by (float)0xffffffff), hence the two min.
__device__ __forceinline__ bool env_header_ok(const EnvView& env)
{
    const EnvHeader* hd = env.header();
    return hd->magic == ENV_MAGIC && hd->width == env.W && hd->height == env.H;
}

// min((uint64)((double)u * (double)sum), sum - 1) for u in [0, 1]; a caller's own random number outside that, or a NaN, is held to
// the ends before the conversion, which is defined for values inside uint64 alone.  sum == 0 (a table of garbage): 0
__device__ __forceinline__ uint64_t env_pick(float u, uint64_t sum)
{
    const double t = (double)u * (double)sum;
    if (!(t > 0.0)) return 0ull;
    if (t >= (double)sum) return sum ? sum - 1ull : 0ull;
    return (uint64_t)t;
}

__device__ __forceinline__ bool env_emit(const EnvView& env, float u, float v, float z, f3& L, f3& E, float& tmax)
{
    const EnvHeader* hd = env.header();
    const uint64_t total = hd->total;
    if (!env_header_ok(env) || total == 0ull) return false;
    const float twoPiOverW = hd->twoPiOverW;
    const uint64_t* __restrict__ M = env.M();
    const uint64_t X = env_pick(u, total);
    uint32_t lo = 0u, hi = env.H - 1u;           // the first row with M[y] > X
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (M[mid] > X) hi = mid; else lo = mid + 1u;
    }
    const uint32_t y = lo;
    const uint64_t below = y ? M[y - 1u] : 0ull, rowSum = M[y] - below;
    const float fy = ((float)(X - below) + 0.5f) / (float)rowSum;
    const uint32_t* __restrict__ Cy = env.C() + (size_t)y * env.W;
    const uint64_t Xc = env_pick(v, rowSum);
    lo = 0u; hi = env.W - 1u;                    // the first column with C[y][x] > Xc
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if ((uint64_t)Cy[mid] > Xc) hi = mid; else lo = mid + 1u;
    }
    const uint32_t x = lo;
    const uint32_t q = Cy[x] - (x ? Cy[x - 1u] : 0u);
    if (q == 0u) return false;
    const float* __restrict__ rowCos = env.rowCos();
    const float c0 = rowCos[y], c1 = rowCos[y + 1u];
    const float ct = c0 + fy * (c1 - c0);
    const float st = sqrtf(cl_max(0.0f, 1.0f - ct * ct));
    const float phi = ((float)x + z) * twoPiOverW;
    L = mk3(st * cosf(phi), ct, st * sinf(phi));
    const float4 texel = env.image[(size_t)y * env.W + x];
    const float s = (((float)total / (float)q) * twoPiOverW) * (c0 - c1);
    E = mk3(texel.x * s, texel.y * s, texel.z * s);
    tmax = 1000.0f;
    return true;
}

// the texel the environment shows along d (rdx_env_lookup, and the depth-0 miss of rdx_trace_paths_env): the row is the band of
// rowCos that holds normalize3(d).y -- the sampling bands --, the column that of atan2f(d.z, d.x); nearest texel, its bits
__device__ __forceinline__ float4 env_lookup(const EnvView& env, const f3& d)
{
    const float4 none = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
    const float inf = __builtin_inff();
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return none;
    if (!(fabsf(d.x) < inf) || !(fabsf(d.y) < inf) || !(fabsf(d.z) < inf) || !env_header_ok(env)) return none;
    const float c = normalize3(d).y;
    const float* __restrict__ rowCos = env.rowCos();
    uint32_t lo = 0u, hi = env.H - 1u;           // the first row whose lower edge lies below c
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rowCos[mid + 1u] < c) hi = mid; else lo = mid + 1u;
    }
    float phi = atan2f(d.z, d.x);
    if (phi < 0.0f) phi = phi + 6.2831855f;
    const uint32_t x = min((uint32_t)(phi * env.header()->wOverTwoPi), env.W - 1u);
    const float4 texel = env.image[(size_t)lo * env.W + x];
    return make_float4(texel.x, texel.y, texel.z, 0.0f);
}

// ---- record ----

// what every light of a shaded point shares: the view vector and the tangent frame of the normal, built once
struct ShadePoint {
    NFrame FN;
    f3 V, N, albedo, above;
    float metallic, roughness, transmission;
};

__device__ __forceinline__ void make_shade_point(ShadePoint& p, const f3& N, const float4& rd, const f3& albedo, float metallic, float roughness,
                                                 float transmission, const f3& above)
{
    p.N = N; p.albedo = albedo; p.above = above;
    p.metallic = metallic; p.roughness = roughness; p.transmission = transmission;
    p.V = normalize3(-mk3(rd.x, rd.y, rd.z));
    make_frame(N, p.FN);
}

// One light's record at `p` from what its emit function returned: the direct term (rgb, 0) and the shadow ray towards it.  A dark
// record is zeros: a shadow ray with tmax 0 accepts nothing.
__device__ __forceinline__ void light_record(bool lit, const ShadePoint& p, const f3& L, const f3& E, float tmax, float4& c, float4& s0, float4& s1)
{
    c = make_float4(0.f, 0.f, 0.f, 0.f); s0 = c; s1 = c;
    if (lit) {
        const f3 direct = mk3(0.0f, 0.0f, 0.0f) + microfacet_brdf(p.FN, L, p.V, p.N, p.albedo, p.metallic, p.roughness, p.transmission) * E;
        c = make_float4(direct.x, direct.y, direct.z, 0.0f);
        s0 = make_float4(p.above.x, p.above.y, p.above.z, 0.001f);
        s1 = make_float4(L.x, L.y, L.z, tmax);
    }
}

// ---- the per-hit kernels ----

// One record per thread: the direction of ray i = rays[2i + 1], material record i = mats[4i .. 4i + 3]; lit[i] = (rgb, 0), shadow
// record i = shadow[2i], shadow[2i + 1] (optional).  emit(i, above, L, E, tmax) is the kernel's light.  Any value of `hit` but 1:
// zeros.  Nothing is gathered, so nothing is fenced; no atomics, no LDS.
template <class Emit>
__device__ __forceinline__ void light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, float4* __restrict__ lit,
                                           float4* __restrict__ shadow, Emit emit)
{
    const uint32_t i = blockIdx.x * LIGHT_HITS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 rd = rays[2 * (size_t)i + 1];
    const float4 m0 = mats[4 * (size_t)i], m1 = mats[4 * (size_t)i + 1], m2 = mats[4 * (size_t)i + 2], m3 = mats[4 * (size_t)i + 3];
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f), s0 = c, s1 = c;
    if (__float_as_uint(m0.w) == 1u) {
        // the light first: its words come through the scalar cache while the record's vector loads are still in flight
        const f3 above = mk3(m3.x, m3.y, m3.z);
        f3 L, E;
        float tmax;
        const bool on = emit(i, above, L, E, tmax);
        ShadePoint p;
        make_shade_point(p, mk3(m0.x, m0.y, m0.z), rd, mk3(m1.x, m1.y, m1.z), m2.x, m2.y, m2.z, above);
        light_record(on, p, L, E, tmax, c, s0, s1);
    }
    lit[i] = c;
    if (shadow) { shadow[2 * (size_t)i] = s0; shadow[2 * (size_t)i + 1] = s1; }
}

} // namespace rdx

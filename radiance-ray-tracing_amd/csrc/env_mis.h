// env_mis.h -- multiple-importance sampling between the environment and the scatter sample (include/rdx.h rdx_env_mis_weights,
// rdx_trace_paths_env_mis): the two densities and the balance-heuristic weight, written ONCE for the per-hit kernel
// and the path kernel (env_mis.hip; their launch declarations are env.h's), so the path call has the bits of the loop over the
// per-hit calls by construction -- the light_emit.h precedent.  The unit is compiled with -ffp-contract=off: every float32 operation is rounded on its own, in the order
// written here; dot3 and normalize3 are those of device_math.h.  numpy float32 restates all of it (tests/env_mis_cases.py).  Device
// code only.
#pragma once
#include "kernels.h"

#include "env.h"
#include "light_emit.h"

namespace rdx {

// the branches of sample_brdf_transm (stages.h) on the same random triple
__device__ __forceinline__ uint32_t lobe_of(const f3& rnd, float transmission)
{
    const bool lower = rnd.z < 0.5f;
    if (lower && (2.0f * rnd.z) < transmission) return LOBE_TRANSMISSION;
    return lower ? LOBE_DIFFUSE : LOBE_SPECULAR;
}

__device__ __forceinline__ bool mis_finite(float v) { return fabsf(v) < __builtin_inff(); }

// The solid-angle density with which the two reflective lobes of sample_brdf_transm together produce L, for NoL = dot3(N, L) > 0:
// d_ggx (stages.h) is the density of ggxTheta, so the specular lobe's is d_ggx NoH / (4 VoH), and acosf(sqrtf(rnd.y)) is
// cosine-weighted.  The lobes are drawn with probability 0.5 and 0.5 (1 - clamp(transmission, 0, 1)).
__device__ __forceinline__ float scatter_pdf(const f3& N, const f3& V, const f3& L, float NoL, float roughness, float transmission)
{
    const f3 H = normalize3(V + L);
    const float NoH = cl_clamp(dot3(N, H), 0.0f, 1.0f);
    const float VoH = cl_clamp(dot3(V, H), 0.0f, 1.0f);
    const float pSpec = d_ggx(NoH, roughness) * NoH / (4.0f * VoH);
    const float pDiff = cl_min(NoL, 1.0f) / RDX_PI;
    const float that = cl_clamp(transmission, 0.0f, 1.0f);
    return 0.5f * pSpec + (0.5f * (1.0f - that)) * pDiff;
}

// The texel (y, x) env_lookup (light_emit.h) shows along d, by its own steps in its own order -- the row is the band of rowCos
// that holds normalize3(d).y, the column that of atan2f(d.z, d.x) --; false where it shows nothing.  A second statement of that
// search and not a function env_lookup calls: taking the search out of env_lookup moves the code of k_env_lookup and k_env_shade
// (profiles/env_mis_kernels.txt), and the existing units stay the ones they were.  y < H and x < W whatever the table holds.
__device__ __forceinline__ bool env_find(const EnvView& env, const f3& d, uint32_t& y, uint32_t& x)
{
    const float inf = __builtin_inff();
    if (d.x == 0.0f && d.y == 0.0f && d.z == 0.0f) return false;
    if (!(fabsf(d.x) < inf) || !(fabsf(d.y) < inf) || !(fabsf(d.z) < inf) || !env_header_ok(env)) return false;
    const float c = normalize3(d).y;
    const float* __restrict__ rowCos = env.rowCos();
    uint32_t lo = 0u, hi = env.H - 1u;           // the first row whose lower edge lies below c
    while (lo < hi) {
        const uint32_t mid = (lo + hi) >> 1;
        if (rowCos[mid + 1u] < c) hi = mid; else lo = mid + 1u;
    }
    float phi = atan2f(d.z, d.x);
    if (phi < 0.0f) phi = phi + 6.2831855f;
    y = lo;
    x = min((uint32_t)(phi * env.header()->wOverTwoPi), env.W - 1u);
    return true;
}

// The solid-angle density with which env_emit produces d: the texel env_lookup shows along d (env_find), its share q / total of
// the table over its solid angle.  0 where the environment shows nothing and where it holds no light.  Every index is env_find's:
// a table of garbage gives an unspecified value, never a read outside the table.
__device__ __forceinline__ float env_pdf(const EnvView& env, const f3& d)
{
    uint32_t y, x;
    if (!env_find(env, d, y, x)) return 0.0f;
    const EnvHeader* hd = env.header();
    const uint64_t total = hd->total;
    if (total == 0ull) return 0.0f;
    const uint32_t* __restrict__ Cy = env.C() + (size_t)y * env.W;
    const uint32_t q = Cy[x] - (x ? Cy[x - 1u] : 0u);
    const float* __restrict__ rowCos = env.rowCos();
    return ((float)q / (float)total) / (hd->twoPiOverW * (rowCos[y] - rowCos[y + 1u]));
}

// what rdx_env_mis_weights writes for one direction
struct MisWeight {
    float w, pScatter, pEnv;
};

// The balance heuristic for direction L seen from a point of normal N and view vector V: w = the weight of the scatter sample, 1 - w
// that of the environment's.  w = 1 -- the environment's sample counts for nothing -- where next-event estimation has no such lobe
// (transmission), where the lobe is a delta (specular at (r r)(r r) == 0), below the horizon of N, and where a density is not finite
// or both are zero.  pScatter is 0 where NoL is not positive.
__device__ __forceinline__ MisWeight env_mis_weight(const EnvView& env, const f3& N, const f3& V, const f3& L, float roughness, float transmission,
                                                    uint32_t lobe)
{
    MisWeight r;
    const float NoL = dot3(N, L);
    const bool up = NoL > 0.0f;
    r.pScatter = up ? scatter_pdf(N, V, L, NoL, roughness, transmission) : 0.0f;
    r.pEnv = env_pdf(env, L);
    const bool delta = lobe == LOBE_SPECULAR && (roughness * roughness) * (roughness * roughness) == 0.0f;
    const float sum = r.pScatter + r.pEnv;
    r.w = 1.0f;
    if (lobe != LOBE_TRANSMISSION && !delta && up && mis_finite(r.pScatter) && mis_finite(r.pEnv) && sum > 0.0f) r.w = r.pScatter / sum;
    return r;
}

} // namespace rdx

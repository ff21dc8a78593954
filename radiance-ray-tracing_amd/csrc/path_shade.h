// path_shade.h -- the shade kernel of one bounce of the path calls (rdx_trace_paths_lights, rdx_trace_paths_punctual,
// rdx_trace_paths_area, rdx_trace_paths_env), written ONCE as a function template over the bounce's light source:
//
//   closest-hit query -> path_shade<Source> -> any-hit query of live x Source::count() shadow rays -> k_lights_fold (light_paths.hip)
//
// It is what rdx_resolve_hits + rdx_resolve_materials + one per-hit light call per light + rdx_scatter_hits compute for a live
// ray, in one pass: the hit is gathered ONCE (hit_material.h), the tangent frame of the normal is built ONCE and serves every light
// (light_emit.h) and the sample.  k_lights_shade, k_punctual_shade, k_area_shade and k_env_shade (light_paths.hip, punctual.hip,
// area.hip, env.hip) are one-line callers with the sources below.  Device code only.
#pragma once
#include "kernels.h"

#include "hit_material.h"
#include "light_emit.h"
#include "light_paths.h"

namespace rdx {

constexpr uint32_t PATH_SHADE_BLOCK = 256;

// ---- the light sources: count() lights, emit(j, above, id, depth, L, E, tmax) = the emit function (light_emit.h) of light j, and
// miss(rd) = what a path whose FIRST ray, of direction rd, hits nothing shows: the stock miss colour (stages.h `environment`).
// Every table is the same address in every lane and the loop counter is uniform, so a record's words arrive through the scalar
// cache and the branch between two tables is uniform.  The tables are the one thing the caller's records can point a kernel at,
// and the host has checked their records into their buffers. ----

// the scene buffer's DirLight array: k_light_hits for light j
__device__ __forceinline__ float4 stock_miss() { return make_float4(0.2f, 0.2f, 0.5f, 0.0f); }

struct DirLightSource {
    const DirLight* __restrict__ lights;
    uint32_t nLights;
    __device__ __forceinline__ uint32_t count() const { return nLights; }
    __device__ __forceinline__ bool emit(uint32_t j, const f3&, const uint4&, uint32_t, f3& L, f3& E, float& tmax) const
    {
        return dir_emit(lights + j, L, E, tmax);
    }
    __device__ __forceinline__ float4 miss(const float4&) const { return stock_miss(); }
};

// a caller's punctual table: k_punctual_light_hits for record j
struct PunctualSource {
    const PunctualLight* __restrict__ lights;
    uint32_t nLights;
    __device__ __forceinline__ uint32_t count() const { return nLights; }
    __device__ __forceinline__ bool emit(uint32_t j, const f3& above, const uint4&, uint32_t, f3& L, f3& E, float& tmax) const
    {
        return punctual_emit(lights + j, above, L, E, tmax);
    }
    __device__ __forceinline__ float4 miss(const float4&) const { return stock_miss(); }
};

// a punctual table, then an area table: after the punctual records, k_area_light_hits for area record a = j - nLights on the keys
// route with stream = a and the path's own (frame, pixel, depth)
struct PunctualAreaSource {
    const PunctualLight* __restrict__ lights;
    uint32_t nLights;
    const AreaLight* __restrict__ area;
    uint32_t nArea;
    __device__ __forceinline__ uint32_t count() const { return nLights + nArea; }
    __device__ __forceinline__ bool emit(uint32_t j, const f3& above, const uint4& id, uint32_t depth, f3& L, f3& E, float& tmax) const
    {
        if (j < nLights) return punctual_emit(lights + j, above, L, E, tmax);
        const uint32_t a = j - nLights;
        const f3 rnd = area_random(id.y, id.z, depth, a);
        return area_emit(area + a, above, rnd.x, rnd.y, L, E, tmax);
    }
    __device__ __forceinline__ float4 miss(const float4&) const { return stock_miss(); }
};

// a punctual table, an area table, then the environment as record nLights + nArea: k_env_light_hits on the keys route with
// stream = nArea and the path's own (frame, pixel, depth).  A first ray that hits nothing shows the environment's texel
struct PunctualAreaEnvSource {
    const PunctualLight* __restrict__ lights;
    uint32_t nLights;
    const AreaLight* __restrict__ area;
    uint32_t nArea;
    EnvView env;
    __device__ __forceinline__ uint32_t count() const { return nLights + nArea + 1u; }
    __device__ __forceinline__ bool emit(uint32_t j, const f3& above, const uint4& id, uint32_t depth, f3& L, f3& E, float& tmax) const
    {
        if (j < nLights) return punctual_emit(lights + j, above, L, E, tmax);
        const uint32_t a = j - nLights;
        const f3 rnd = area_random(id.y, id.z, depth, a);
        if (a < nArea) return area_emit(area + a, above, rnd.x, rnd.y, L, E, tmax);
        return env_emit(env, rnd.x, rnd.y, rnd.z, L, E, tmax);
    }
    __device__ __forceinline__ float4 miss(const float4& rd) const { return env_lookup(env, mk3(rd.x, rd.y, rd.z)); }
};

// One live ray per lane.  A hit that fails gather_hit is a miss and is counted -- one ballot per wave, one atomic by its first
// lane, and only where the wave has such a hit.  The survivors are compacted by k_scatter_hits' rule -- the survivors of 64
// consecutive live rays stay together and in order: a lane's record is the block's base from ONE atomic on *live per BLOCK, plus
// the survivors of the block's earlier waves, plus the lane's rank in its wave's ballot.  Survivor k writes the records k * count()
// + j of its lights, ray-major.  20 bytes of LDS: the block's four survivor counts and its base.
//
// Mis is what rdx_trace_paths_env_mis adds (env_mis.hip EnvMis): the LAST record of the source is the environment and
// is weighted by 1 - skyWeight of its direction wherever a next ray is sampled, scatterWeight of the sampled direction travels in
// foldF.w -- the fold hands it on in nWeight.w, where this kernel finds it as w.w at the next depth --, and a live ray of depth > 0
// without a valid hit adds weight * (source.miss(rd) * w.w) to its path's colour.  NoMis is every other call's: `on` is a
// compile-time false and nothing of this is in their code.
struct NoMis {
    static constexpr bool on = false;
};

template <class Source, class Mis = NoMis>
__device__ __forceinline__ void path_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, const ShadeScene& sc,
                                           const Source& source, const LightPathStreams& io, uint32_t n, uint32_t depth, uint32_t sampleNext,
                                           uint32_t* __restrict__ live, uint32_t* __restrict__ invalid, const Mis& mis = Mis{})
{
    const uint32_t i = blockIdx.x * PATH_SHADE_BLOCK + threadIdx.x;
    bool alive = false, bad = false;
    uint4 id = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro, ha = ro;
    HitGather g = {0u, 0u, 0xffffffffu, {0u, 0u, 0u}};
    if (i < n) {
        ro = io.rays[2 * (size_t)i]; rd = io.rays[2 * (size_t)i + 1];
        ha = io.hits[2 * (size_t)i];
        const float4 hb = io.hits[2 * (size_t)i + 1];
        if (depth == 0u) {
            const uint4 key = io.keys[i];
            id = make_uint4(i, key.x, key.y, 0u);
        } else {
            id = io.ids[i];
            w = io.weight[i];
        }
        if (__float_as_uint(ha.w) == 1u) {
            alive = gather_hit(sc, slotOf, nInst, hb, g);
            bad = !alive;
        }
        // a path's colour starts at zero; a miss at depth 0 shows what the source shows there
        if (depth == 0u) {
            float4 first = make_float4(0.0f, 0.0f, 0.0f, 0.0f);
            if (!alive) first = source.miss(rd);
            io.radiance[i] = first;
        }
        if constexpr (Mis::on) {
            // the scatter sample that found the environment.  A path has one live ray and the fold of depth - 1 precedes this launch in
            // stream order: a plain load and store
            if (depth != 0u && !alive) {
                const float4 sky = source.miss(rd);
                const float4 c = io.radiance[id.x];
                const f3 color = mk3(c.x, c.y, c.z) + mk3(w.x, w.y, w.z) * (mk3(sky.x, sky.y, sky.z) * w.w);
                io.radiance[id.x] = make_float4(color.x, color.y, color.z, 0.0f);
            }
        }
    }
    // wave64 ballots: every lane of the wave is here (no thread has returned)
    const unsigned long long mb = __ballot(bad);
    if (mb != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (uint32_t)__popcll(mb));
    const unsigned long long m = __ballot(alive);
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    // the block's four ballots are summed in LDS and the cursor moves ONCE per block, as k_shade does (kernels.hip): the
    // device-scope atomics of all waves land on one word and serialise, about 11.5 ns each, which at one per wave
    // was most of this kernel's time.  The survivors of a block are contiguous and its waves in order, which keeps the rule.
    __shared__ uint32_t s_count[PATH_SHADE_BLOCK / 64], s_base;
    if (lane == 0u) s_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t v = 0; v < PATH_SHADE_BLOCK / 64; ++v) total += s_count[v];
        s_base = total ? atomicAdd(live, total) : 0u;
    }
    __syncthreads();
    if (!alive) return;
    uint32_t base = s_base;
    for (uint32_t v = 0; v < wave; ++v) base += s_count[v];
    const size_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));

    // ---- the material record of k_resolve_materials and the `below` of k_resolve_hits, in registers; one frame for all lights and
    // the sample (the per-hit kernels and k_scatter_hits each build this one from the record's N) ----
    HitMaterial mat;
    eval_hit_material(sc, insts, ro, rd, ha, g, mat);
    ShadePoint p;
    make_shade_point(p, mat.N, rd, mat.albedo, mat.metallic, mat.roughness, mat.transmission, mat.above);

    // ---- the per-hit light call of every light of the source: ONE rolled loop, so microfacet_brdf is in the code once ----
    const uint32_t nAll = source.count();
    const size_t first = k * nAll;
#pragma unroll 1
    for (uint32_t j = 0; j < nAll; ++j) {
        f3 L, E;
        float tmax;
        const bool lit = source.emit(j, mat.above, id, depth, L, E, tmax);
        float4 c, s0, s1;
        light_record(lit, p, L, E, tmax, c, s0, s1);
        if constexpr (Mis::on) {
            // a uniform branch on j and the depth: the weight is evaluated for the environment's record alone, and only where a next
            // ray is sampled -- at the last depth no scatter sample carries the other share, and the record counts in full
            if (j + 1u == nAll && sampleNext && lit) {
                const float ws = 1.0f - mis.skyWeight(p, L);
                c = make_float4(c.x * ws, c.y * ws, c.z * ws, 0.0f);
            }
        }
        const size_t r = first + j;
        io.lit[r] = c;
        io.shadow[2 * r] = s0;
        io.shadow[2 * r + 1] = s1;
    }

    // ---- k_scatter_hits with the key (frameID, pixel, depth) ----
    f3 nf = mk3(0.f, 0.f, 0.f);
    float wNext = 0.0f;
    if (sampleNext) {
        const f3 rnd = pcg3d(id.y, id.z, depth);
        const f3 nd = sample_brdf_transm(p.FN, p.V, mat.N, mat.albedo, mat.metallic, mat.roughness, mat.transmission, mat.ior, rnd, nf);
        if constexpr (Mis::on) wNext = mis.scatterWeight(p, nd, rnd);
        const f3 origin = dot3(nd, mat.N) < 0 ? mat.below : mat.above;      // getHitPosition(hitData, -+faceN)
        io.nRays[2 * k] = make_float4(origin.x, origin.y, origin.z, 0.001f);
        io.nRays[2 * k + 1] = make_float4(nd.x, nd.y, nd.z, 1000.0f);
    }
    const f3 ambient = mat.albedo * 0.1f;
    io.nIds[k] = id;
    io.nWeight[k] = w;
    io.foldF[k] = make_float4(nf.x, nf.y, nf.z, wNext);
    io.foldA[k] = make_float4(ambient.x, ambient.y, ambient.z, 0.0f);
}

} // namespace rdx

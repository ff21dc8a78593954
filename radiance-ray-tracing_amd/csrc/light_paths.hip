// light_paths.hip -- device side of rdx_trace_paths_lights: one bounce of a path tracer that samples EVERY directional light of the
// scene at every hit, fused into two kernels around the any-hit query of the bounce's shadow rays (include/rdx.h).
//
//   closest-hit query -> k_lights_shade -> any-hit query of live x L shadow rays -> k_lights_fold
//
// k_lights_shade is what rdx_resolve_hits + rdx_resolve_materials + L x rdx_light_hits + rdx_scatter_hits compute for a live ray,
// in one pass: the hit is gathered ONCE, the tangent frame of the normal is built ONCE and serves every light and the sample.
//
// A translation unit of its own, like surface.hip, shade.hip, material.hip and scatter.hip and for the same reason: the code
// objects of kernels.hip, surface.hip, shade.hip, material.hip, scatter.hip, paths.hip, raygen.hip and tlas_update.hip stay the ones
// they were, bit for bit (profiles/light_paths_kernels.txt).  The gather part is restated operation for operation from
// k_resolve_materials (material.hip); the PBR, frame and RNG functions are those of stages.h / device_math.h, called as
// k_light_hits (material.hip) and k_scatter_hits (scatter.hip) call them.
#include "kernels.h"

#include "device_math.h"
#include "light_paths.h"
#include "shade.h"
#include "stages.h"
#include "surface.h"

namespace rdx {

constexpr uint32_t LIGHT_PATHS_BLOCK = 256;

// One live ray per lane.  Every gather of a hit is fenced by shade_in_bounds (shade.h), asked before and after the index gather
// exactly as k_resolve_materials asks it, plus the slotOf check; a hit that fails is a miss and is counted -- one ballot per wave,
// one atomic by its first lane, and only where the wave has such a hit.  The survivors are compacted by k_scatter_hits' rule --
// the survivors of 64 consecutive live rays stay together and in order: a lane's record is the block's base from ONE atomic on
// *live per BLOCK, plus the survivors of the block's earlier waves, plus the lane's rank in its wave's ballot.  `lights` is the
// scene buffer's DirLight array: the same address in every lane and a loop counter that is uniform, so each light's eight floats
// arrive through the scalar cache; the loop stays rolled, so microfacet_brdf is in the code once.  20 bytes of LDS: the block's
// four survivor counts and its base.
__global__ void __launch_bounds__(LIGHT_PATHS_BLOCK)
k_lights_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc, const DirLight* __restrict__ lights,
               uint32_t nLights, LightPathStreams io, uint32_t n, uint32_t depth, uint32_t sampleNext, uint32_t* __restrict__ live,
               uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * LIGHT_PATHS_BLOCK + threadIdx.x;
    bool alive = false, bad = false;
    uint4 id = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro, ha = ro;
    uint32_t prim = 0u, inst = 0u, slot = 0xffffffffu, idx[3] = {0u, 0u, 0u};
    const bool texOn = (sc.tex.flags & TEX_ENABLED) != 0u;
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
            prim = __float_as_uint(hb.x); inst = __float_as_uint(hb.y);
            bool ok = shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, nullptr, sc.s.nIndex, sc.s.nNormal, sc.s.nUv, sc.materials,
                                      sc.nMaterials, texOn, sc.tex.layers);
            if (ok) {
                slot = slotOf[inst];        // 0xffffffff: no instance of the TLAS carries this index (a foreign blob)
                const int64_t first = (int64_t)sc.s.meshInfo[inst].indexOffset + (int64_t)prim * 3;
                idx[0] = sc.s.index[first]; idx[1] = sc.s.index[first + 1]; idx[2] = sc.s.index[first + 2];
                ok = slot < nInst && shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, idx, sc.s.nIndex, sc.s.nNormal, sc.s.nUv,
                                                     sc.materials, sc.nMaterials, texOn, sc.tex.layers);
            }
            alive = ok;
            bad = !ok;
        }
        // a path's colour starts at zero; a miss at depth 0 shows the stock miss colour (stages.h `environment`)
        if (depth == 0u) io.radiance[i] = alive ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(0.2f, 0.2f, 0.5f, 0.0f);
    }
    // wave64 ballots: every lane of the wave is here (no thread has returned)
    const unsigned long long mb = __ballot(bad);
    if (mb != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (uint32_t)__popcll(mb));
    const unsigned long long m = __ballot(alive);
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    // the block's four ballots are summed in LDS and the cursor moves ONCE per block, as k_shade does (kernels.hip): the
    // device-scope atomics of all waves land on one word and serialise, about 11.5 ns each, which at one per wave
    // was most of this kernel's time.  The survivors of a block are contiguous and its waves in order, which keeps the rule.
    __shared__ uint32_t s_count[LIGHT_PATHS_BLOCK / 64], s_base;
    if (lane == 0u) s_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t v = 0; v < LIGHT_PATHS_BLOCK / 64; ++v) total += s_count[v];
        s_base = total ? atomicAdd(live, total) : 0u;
    }
    __syncthreads();
    if (!alive) return;
    uint32_t base = s_base;
    for (uint32_t v = 0; v < wave; ++v) base += s_count[v];
    const size_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));

    // ---- the material record of k_resolve_materials and the `below` of k_resolve_hits, in registers ----
    const MeshInfo mi = sc.s.meshInfo[inst];
    const Material mt = sc.materials[mi.materialIndex];
    const DInst& I = insts[slot];
    // HitData.hitPoint = localOrigin + localDir * t and barycentric, as kernels.hip fill_hit_info (radiance.cl:243)
    HitInfo h;
    const f3 lo = mat4_mul3(I.inv, ro.x, ro.y, ro.z, 1.0f);
    const f3 ld = mat4_mul3(I.inv, rd.x, rd.y, rd.z, 0.0f);
    h.hitPoint = lo + ld * ha.x;
    h.bx = 1 - ha.y - ha.z; h.by = ha.y; h.bz = ha.z;
    h.primitiveIndex = prim;
    h.instanceIndex = inst;
    h.fwd = I.fwd;
    // interpolated vertex normal -> world by the object->world matrix, w = 0 (shader.cl:340-368); the positions are those
    // shade_in_bounds proved inside, in 64 bits
    const float* nb = sc.s.normal + (int64_t)mi.normalOffset;
    const int64_t v0 = (int64_t)idx[0] * 3, v1 = (int64_t)idx[1] * 3, v2 = (int64_t)idx[2] * 3;
    const f3 n0 = mk3(nb[v0], nb[v0 + 1], nb[v0 + 2]);
    const f3 n1 = mk3(nb[v1], nb[v1 + 1], nb[v1 + 2]);
    const f3 n2 = mk3(nb[v2], nb[v2 + 1], nb[v2 + 2]);
    const f3 nl = mk3(h.bx * n0.x + h.by * n1.x + h.bz * n2.x, h.bx * n0.y + h.by * n1.y + h.bz * n2.y,
                      h.bx * n0.z + h.by * n1.z + h.bz * n2.z);
    const float nw = h.bx * 0.0f + h.by * 0.0f + h.bz * 0.0f;
    const f3 faceN = normalize3(mat4_mul3(h.fwd, nl.x, nl.y, nl.z, nw));
    // getHitPosition(hitData, +-faceN) (shader.cl:453-468): transform * (hitPoint, 1), pushed off the surface along N and along -N
    const f3 P = mat4_mul3(h.fwd, h.hitPoint.x, h.hitPoint.y, h.hitPoint.z, 1.0f);
    const f3 above = P + faceN * 0.00001f;
    const f3 below = P + (-faceN) * 0.00001f;

    // texels are read only when option "textures" is on and an image array is given (TEX_ENABLED); otherwise a material with a
    // texture index sees texel 0, as in the live reference shader (stages.h:255-257)
    float tu = 0.0f, tv = 0.0f;
    if (texOn) {     // getUV, shader.cl:323-338
        const float* ub = sc.s.uv + (int64_t)mi.uvOffset;
        tu = h.bx * ub[v0] + h.by * ub[v1] + h.bz * ub[v2];
        tv = h.bx * ub[v0 + 1] + h.by * ub[v1 + 1] + h.bz * ub[v2 + 1];
    }
    f3 N = faceN;       // getMatNormal, shader.cl:369-395
    if (mt.normalTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.normalTexIdx, tx);
        f4 t; t.x = cl_clamp((float)tx[0] / 255.0f, 0.0f, 1.0f) * 2.0f - 1.0f; t.y = cl_clamp((float)tx[1] / 255.0f, 0.0f, 1.0f) * 2.0f - 1.0f;
        t.z = cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f) * 2.0f - 1.0f; t.w = 0.0f * 2.0f - 1.0f;
        t = normalize4(t);
        float tbn[16];
        normal_space(faceN, tbn);
        N = normalize3(mat4_mul3(tbn, t.x, t.y, t.z, t.w));
    }
    float metallic = mt.metallic;       // getMaterialProp, shader.cl:398-430
    if (mt.metallicTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.metallicTexIdx, tx);
        metallic = cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f);                   // .z (shader.cl:412)
    }
    float roughness = cl_clamp(mt.roughness, 0.0f, 1.0f);
    if (mt.roughnessTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.roughnessTexIdx, tx);
        roughness = cl_clamp((float)tx[1] / 255.0f, 0.05f, 1.0f);                 // .y (shader.cl:422)
    }
    const float transmission = cl_clamp(mt.transmission, 0.0f, 1.0f);
    const float ior = cl_clamp(mt.ior, 0.0f, 10.0f);
    f3 albedo = mk3(mt.albedo[0], mt.albedo[1], mt.albedo[2]);       // getAlbedo, shader.cl:432-451
    if (mt.albedoTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.albedoTexIdx, tx);
        albedo = mk3(cl_clamp((float)tx[0] / 255.0f, 0.0f, 1.0f), cl_clamp((float)tx[1] / 255.0f, 0.0f, 1.0f), cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f));
    }

    // ---- one frame for all lights and the sample (k_light_hits and k_scatter_hits each build this one from the record's N) ----
    const f3 V = normalize3(-mk3(rd.x, rd.y, rd.z));
    NFrame FN;
    make_frame(N, FN);

    // ---- k_light_hits for light j = 0 .. L - 1: records k * L + j, ray-major ----
#pragma unroll 1
    for (uint32_t j = 0; j < nLights; ++j) {
        const DirLight* light = lights + j;
        const f3 L = normalize3(mk3(-light->direction[0], -light->direction[1], -light->direction[2]));
        const f3 direct = mk3(0.0f, 0.0f, 0.0f) + microfacet_brdf(FN, L, V, N, albedo, metallic, roughness, transmission) *
                                                  mk3(light->color[0], light->color[1], light->color[2]);
        const size_t r = k * nLights + j;
        io.lit[r] = make_float4(direct.x, direct.y, direct.z, 0.0f);
        io.shadow[2 * r] = make_float4(above.x, above.y, above.z, 0.001f);
        io.shadow[2 * r + 1] = make_float4(L.x, L.y, L.z, 1000.0f);
    }

    // ---- k_scatter_hits with the key (frameID, pixel, depth) ----
    f3 nf = mk3(0.f, 0.f, 0.f);
    if (sampleNext) {
        const f3 rnd = pcg3d(id.y, id.z, depth);
        const f3 nd = sample_brdf_transm(FN, V, N, albedo, metallic, roughness, transmission, ior, rnd, nf);
        const f3 origin = dot3(nd, N) < 0 ? below : above;      // getHitPosition(hitData, -+faceN)
        io.nRays[2 * k] = make_float4(origin.x, origin.y, origin.z, 0.001f);
        io.nRays[2 * k + 1] = make_float4(nd.x, nd.y, nd.z, 1000.0f);
    }
    const f3 ambient = albedo * 0.1f;
    io.nIds[k] = id;
    io.nWeight[k] = w;
    io.foldF[k] = make_float4(nf.x, nf.y, nf.z, 0.0f);
    io.foldA[k] = make_float4(ambient.x, ambient.y, ambient.z, 0.0f);
}

// One survivor per lane.  A path has at most one live ray, so radiance[path] and the weight are plain loads and stores: no atomics,
// no LDS.  Every float32 operation is rounded on its own (this unit is compiled with -ffp-contract=off), in the order of the
// README's loop: direct = ((0 + x_0) + x_1) + ..., x_j = occluded ? 0 : lit_j; radiance = direct + ambient; color += weight *
// radiance; weight *= nextFactor.
__global__ void __launch_bounds__(LIGHT_PATHS_BLOCK)
k_lights_fold(const float4* __restrict__ any, uint32_t nLights, LightPathStreams io, uint32_t n)
{
    const uint32_t k = blockIdx.x * LIGHT_PATHS_BLOCK + threadIdx.x;
    if (k >= n) return;
    f3 direct = mk3(0.0f, 0.0f, 0.0f);
#pragma unroll 1
    for (uint32_t j = 0; j < nLights; ++j) {
        const size_t r = (size_t)k * nLights + j;
        const bool occluded = __float_as_uint(any[2 * r].w) == 1u;
        const float4 l = io.lit[r];
        direct = direct + (occluded ? mk3(0.0f, 0.0f, 0.0f) : mk3(l.x, l.y, l.z));
    }
    const float4 a = io.foldA[k], f = io.foldF[k], w = io.nWeight[k];
    const uint32_t path = io.nIds[k].x;
    const f3 radiance = direct + mk3(a.x, a.y, a.z);
    const float4 c = io.radiance[path];
    const f3 weight = mk3(w.x, w.y, w.z);
    const f3 color = mk3(c.x, c.y, c.z) + weight * radiance;
    const f3 next = weight * mk3(f.x, f.y, f.z);
    io.radiance[path] = make_float4(color.x, color.y, color.z, 0.0f);
    io.nWeight[k] = make_float4(next.x, next.y, next.z, 0.0f);
}

void launch_lights_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const DirLight* lights,
                         uint32_t nLights, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext, uint32_t* live,
                         uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LIGHT_PATHS_BLOCK - 1) / LIGHT_PATHS_BLOCK);
    hipLaunchKernelGGL(k_lights_shade, dim3(blocks), dim3(LIGHT_PATHS_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, io, n, depth,
                       sampleNext ? 1u : 0u, live, invalid);
}

void launch_lights_fold(hipStream_t st, const float4* any, uint32_t nLights, const LightPathStreams& io, uint32_t live)
{
    if (!live) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)live + LIGHT_PATHS_BLOCK - 1) / LIGHT_PATHS_BLOCK);
    hipLaunchKernelGGL(k_lights_fold, dim3(blocks), dim3(LIGHT_PATHS_BLOCK), 0, st, any, nLights, io, live);
}

} // namespace rdx

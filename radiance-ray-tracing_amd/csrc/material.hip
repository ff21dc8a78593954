// material.hip -- device side of rdx_resolve_materials and rdx_light_hits: what the stock closest-hit shader `material` (stages.h)
// evaluates before its light term, as a record per hit, and that light term for any one of the scene's directional lights
// (include/rdx.h rdx_material_record).
//
// A translation unit of its own, like surface.hip and shade.hip and for the same reason: the code objects of kernels.hip,
// surface.hip, shade.hip and paths.hip stay the ones they were, bit for bit (profiles/material_kernels.txt).  The PBR functions
// are those of stages.h, called as `material` calls them; the gather part of `material` (stages.h:235-299) and the HitInfo
// derivation (shade.hip) are restated here, operation for operation, so that neither is touched.
#include "kernels.h"

#include "device_math.h"
#include "material_eval.h"
#include "shade.h"
#include "stages.h"
#include "surface.h"

namespace rdx {

constexpr uint32_t MATERIAL_BLOCK = 256;

// One ray per thread: ray i = rays[2i], rays[2i + 1], record i = hits[2i], hits[2i + 1] (as k_shade_hits), material record i =
// out[4i .. 4i + 3]: adjacent lanes read adjacent 32-byte records and write adjacent 64-byte ones.  Every gather of a hit is fenced
// by shade_in_bounds (shade.h), asked before and after the index gather exactly as k_shade_hits asks it; a record that fails it
// writes zeros and is counted -- one ballot per wave, one atomic by its first lane, and only where the wave has such a record.
__global__ void __launch_bounds__(MATERIAL_BLOCK)
k_resolve_materials(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, const float4* __restrict__ rays,
                    const float4* __restrict__ hits, uint32_t n, ShadeScene sc, float4* __restrict__ out, uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * MATERIAL_BLOCK + threadIdx.x;
    bool bad = false;
    if (i < n) {
        const float4 ro = rays[2 * (size_t)i], rd = rays[2 * (size_t)i + 1];
        const float4 ha = hits[2 * (size_t)i], hb = hits[2 * (size_t)i + 1];
        float4 r0 = make_float4(0.f, 0.f, 0.f, 0.f), r1 = r0, r2 = r0, r3 = r0;
        if (__float_as_uint(ha.w) == 1u) {
            const uint32_t prim = __float_as_uint(hb.x), inst = __float_as_uint(hb.y);
            const bool texOn = (sc.tex.flags & TEX_ENABLED) != 0u;
            uint32_t slot = 0xffffffffu, idx[3] = {0u, 0u, 0u};
            bool ok = shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, nullptr, sc.s.nIndex, sc.s.nNormal, sc.s.nUv, sc.materials,
                                      sc.nMaterials, texOn, sc.tex.layers);
            if (ok) {
                slot = slotOf[inst];        // 0xffffffff: no instance of the TLAS carries this index (a foreign blob)
                const int64_t first = (int64_t)sc.s.meshInfo[inst].indexOffset + (int64_t)prim * 3;
                idx[0] = sc.s.index[first]; idx[1] = sc.s.index[first + 1]; idx[2] = sc.s.index[first + 2];
                ok = slot < nInst && shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, idx, sc.s.nIndex, sc.s.nNormal, sc.s.nUv,
                                                     sc.materials, sc.nMaterials, texOn, sc.tex.layers);
            }
            if (ok) {
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
                const f3 hitPos = offset_hit_position(h, faceN);        // getHitPosition(hitData, faceN): the shadow ray's origin

                // texels are read only when option "textures" is on and an image array is given (TEX_ENABLED); otherwise a material
                // with a texture index sees texel 0, as in the live reference shader (stages.h:255-257)
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
                r0 = make_float4(N.x, N.y, N.z, __uint_as_float(1u));
                r1 = make_float4(albedo.x, albedo.y, albedo.z, __uint_as_float((uint32_t)mi.materialIndex));
                r2 = make_float4(metallic, roughness, transmission, ior);
                r3 = make_float4(hitPos.x, hitPos.y, hitPos.z, 0.0f);
            } else {
                bad = true;
            }
        }
        float4* o = out + 4 * (size_t)i;
        o[0] = r0; o[1] = r1; o[2] = r2; o[3] = r3;
    }
    // wave64 ballot: every lane of the wave is here (no thread has returned)
    const unsigned long long m = __ballot(bad);
    if (m != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (uint32_t)__popcll(m));
}

// One record per thread: the direction of ray i = rays[2i + 1], material record i = mats[4i .. 4i + 3]; lit[i] = (rgb, 0), shadow
// record i = shadow[2i], shadow[2i + 1].  `light` is one DirLight of the scene buffer: the same address in every lane, so its eight
// floats arrive through the scalar cache.  The arithmetic is the light term of `material` (stages.h:276-278, 309-312) with that
// light in the place of lights[0].  Nothing is gathered, so nothing is fenced; no atomics, no LDS.
__global__ void __launch_bounds__(MATERIAL_BLOCK)
k_light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, const DirLight* __restrict__ light,
             float4* __restrict__ lit, float4* __restrict__ shadow)
{
    const uint32_t i = blockIdx.x * MATERIAL_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 rd = rays[2 * (size_t)i + 1];
    const float4 m0 = mats[4 * (size_t)i], m1 = mats[4 * (size_t)i + 1], m2 = mats[4 * (size_t)i + 2], m3 = mats[4 * (size_t)i + 3];
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f), s0 = c, s1 = c;      // any other value of `hit`: zeros (a shadow ray with tmax 0 accepts nothing)
    if (__float_as_uint(m0.w) == 1u) {
        const f3 N = mk3(m0.x, m0.y, m0.z), albedo = mk3(m1.x, m1.y, m1.z);
        const float metallic = m2.x, roughness = m2.y, transmission = m2.z;
        const f3 L = normalize3(mk3(-light->direction[0], -light->direction[1], -light->direction[2]));
        const f3 V = normalize3(-mk3(rd.x, rd.y, rd.z));
        NFrame FN;
        make_frame(N, FN);
        const f3 direct = mk3(0.0f, 0.0f, 0.0f) + microfacet_brdf(FN, L, V, N, albedo, metallic, roughness, transmission) *
                                                  mk3(light->color[0], light->color[1], light->color[2]);
        c = make_float4(direct.x, direct.y, direct.z, 0.0f);
        s0 = make_float4(m3.x, m3.y, m3.z, 0.001f);
        s1 = make_float4(L.x, L.y, L.z, 1000.0f);
    }
    lit[i] = c;
    if (shadow) { shadow[2 * (size_t)i] = s0; shadow[2 * (size_t)i + 1] = s1; }
}

void launch_resolve_materials(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits,
                              uint32_t n, const ShadeScene& sc, float4* out, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + MATERIAL_BLOCK - 1) / MATERIAL_BLOCK);
    hipLaunchKernelGGL(k_resolve_materials, dim3(blocks), dim3(MATERIAL_BLOCK), 0, st, insts, slotOf, nInst, rays, hits, n, sc, out, invalid);
}

void launch_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const DirLight* light, float4* lit, float4* shadow)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + MATERIAL_BLOCK - 1) / MATERIAL_BLOCK);
    hipLaunchKernelGGL(k_light_hits, dim3(blocks), dim3(MATERIAL_BLOCK), 0, st, rays, materials, n, light, lit, shadow);
}

} // namespace rdx

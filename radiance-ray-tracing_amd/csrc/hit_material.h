// hit_material.h -- the two steps every device-resident shading call takes from a closest-hit query record to an evaluated
// material, each written ONCE: the fenced gather of the hit, and what the stock closest-hit shader `material` (stages.h) evaluates
// before its light term.  k_resolve_materials (material.hip) writes the result out as a record; the shade kernels of the path calls
// (path_shade.h) keep it in registers.  Device code only.
//
// The PBR functions are those of stages.h, called as `material` calls them; the gather part of `material` (stages.h:235-299) and the
// HitInfo derivation (shade.hip) are restated here, operation for operation, so that neither is touched: stages.h is the
// benchmark's hot path and kernels.hip keeps its machine code.  The units that include this header are compiled with
// -ffp-contract=off: every float32 operation below is rounded on its own, and the sums are written out by hand because numpy
// restates them (tests/material_cases.py).
#pragma once
#include "kernels.h"

#include "device_math.h"
#include "shade.h"
#include "stages.h"
#include "surface.h"

namespace rdx {

// what a valid hit record points at: the primitive, the instance, the TLAS slot that carries the instance, the three vertex indices
struct HitGather { uint32_t prim, inst, slot, idx[3]; };

// The fenced gather of the record whose second half is `hb`.  shade_in_bounds (shade.h) is asked before and after the index gather
// exactly as k_shade_hits asks it, and slotOf must name a slot of the TLAS; false: something the record points at lies outside a
// buffer, and nothing behind it may be read.  `g` is whole either way (slot 0xffffffff, indices 0 where the gather stopped).
__device__ __forceinline__ bool gather_hit(const ShadeScene& sc, const uint32_t* __restrict__ slotOf, uint32_t nInst, const float4& hb, HitGather& g)
{
    const bool texOn = (sc.tex.flags & TEX_ENABLED) != 0u;
    g.prim = __float_as_uint(hb.x); g.inst = __float_as_uint(hb.y);
    g.slot = 0xffffffffu; g.idx[0] = 0u; g.idx[1] = 0u; g.idx[2] = 0u;
    bool ok = shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, g.inst, g.prim, nullptr, sc.s.nIndex, sc.s.nNormal, sc.s.nUv, sc.materials,
                              sc.nMaterials, texOn, sc.tex.layers);
    if (ok) {
        g.slot = slotOf[g.inst];        // 0xffffffff: no instance of the TLAS carries this index (a foreign blob)
        const int64_t first = (int64_t)sc.s.meshInfo[g.inst].indexOffset + (int64_t)g.prim * 3;
        g.idx[0] = sc.s.index[first]; g.idx[1] = sc.s.index[first + 1]; g.idx[2] = sc.s.index[first + 2];
        ok = g.slot < nInst && shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, g.inst, g.prim, g.idx, sc.s.nIndex, sc.s.nNormal, sc.s.nUv,
                                               sc.materials, sc.nMaterials, texOn, sc.tex.layers);
    }
    return ok;
}

// the evaluated material of one hit (include/rdx.h rdx_material_record, plus the face normal and `below` of rdx_surface)
struct HitMaterial {
    f3 N, faceN, albedo;
    float metallic, roughness, transmission, ior;
    f3 above, below;            // getHitPosition(hitData, +-faceN): the hit point pushed off the surface along N and along -N
    int32_t materialIndex;
};

// The material of the hit (ro, rd, ha) whose gather `g` succeeded.  A caller that does not use a field pays nothing for it.
__device__ __forceinline__ void eval_hit_material(const ShadeScene& sc, const DInst* __restrict__ insts, const float4& ro, const float4& rd,
                                                  const float4& ha, const HitGather& g, HitMaterial& m)
{
    const bool texOn = (sc.tex.flags & TEX_ENABLED) != 0u;
    const MeshInfo mi = sc.s.meshInfo[g.inst];
    const Material mt = sc.materials[mi.materialIndex];
    const DInst& I = insts[g.slot];
    // HitData.hitPoint = localOrigin + localDir * t and barycentric, as kernels.hip fill_hit_info (radiance.cl:243)
    HitInfo h;
    const f3 lo = mat4_mul3(I.inv, ro.x, ro.y, ro.z, 1.0f);
    const f3 ld = mat4_mul3(I.inv, rd.x, rd.y, rd.z, 0.0f);
    h.hitPoint = lo + ld * ha.x;
    h.bx = 1 - ha.y - ha.z; h.by = ha.y; h.bz = ha.z;
    h.primitiveIndex = g.prim;
    h.instanceIndex = g.inst;
    h.fwd = I.fwd;
    // interpolated vertex normal -> world by the object->world matrix, w = 0 (shader.cl:340-368); the positions are those
    // shade_in_bounds proved inside, in 64 bits
    const float* nb = sc.s.normal + (int64_t)mi.normalOffset;
    const int64_t v0 = (int64_t)g.idx[0] * 3, v1 = (int64_t)g.idx[1] * 3, v2 = (int64_t)g.idx[2] * 3;
    const f3 n0 = mk3(nb[v0], nb[v0 + 1], nb[v0 + 2]);
    const f3 n1 = mk3(nb[v1], nb[v1 + 1], nb[v1 + 2]);
    const f3 n2 = mk3(nb[v2], nb[v2 + 1], nb[v2 + 2]);
    const f3 nl = mk3(h.bx * n0.x + h.by * n1.x + h.bz * n2.x, h.bx * n0.y + h.by * n1.y + h.bz * n2.y,
                      h.bx * n0.z + h.by * n1.z + h.bz * n2.z);
    const float nw = h.bx * 0.0f + h.by * 0.0f + h.bz * 0.0f;
    const f3 faceN = normalize3(mat4_mul3(h.fwd, nl.x, nl.y, nl.z, nw));
    // getHitPosition(hitData, +-faceN) (shader.cl:453-468): transform * (hitPoint, 1), pushed off the surface along N and along -N
    const f3 P = mat4_mul3(h.fwd, h.hitPoint.x, h.hitPoint.y, h.hitPoint.z, 1.0f);
    m.above = P + faceN * 0.00001f;
    m.below = P + (-faceN) * 0.00001f;

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
    f3 albedo = mk3(mt.albedo[0], mt.albedo[1], mt.albedo[2]);       // getAlbedo, shader.cl:432-451
    if (mt.albedoTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.albedoTexIdx, tx);
        albedo = mk3(cl_clamp((float)tx[0] / 255.0f, 0.0f, 1.0f), cl_clamp((float)tx[1] / 255.0f, 0.0f, 1.0f), cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f));
    }
    m.N = N; m.faceN = faceN; m.albedo = albedo;
    m.metallic = metallic; m.roughness = roughness;
    m.transmission = cl_clamp(mt.transmission, 0.0f, 1.0f);
    m.ior = cl_clamp(mt.ior, 0.0f, 10.0f);
    m.materialIndex = mi.materialIndex;
}

} // namespace rdx

// shade.h -- what rdx_shade_hits shares between the host runtime, its kernel (shade.hip) and the CPU tests: the view of the scene
// buffers with their element counts, and the bounds rule of one hit record -- surface_in_bounds (surface.h) extended by what the
// closest-hit shader `material` (stages.h) reads beyond the surface record: its Material, and that Material's texture layers.
// Compiles for host and device.
#pragma once
#include <stdint.h>

#include "rdx_types.h"
#include "surface.h"
#include "texture.h"

namespace rdx {

struct ShadeScene {                // descriptor slots 4, 5, 7, 8, 9, 10, 11 + 12 with their ELEMENT counts
    SurfaceScene s;                // slots 5, 7, 8, 9; s.uv / s.nUv are set only when textures are on (nothing else reads the uv stream)
    const SceneProperties* scene;  // slot 4, a whole SceneProperties
    const Material* materials;     // slot 10
    uint32_t nMaterials;
    TexView tex;                   // slots 11 + 12: TEX_ENABLED only when option "textures" is 1 and an image array is given
};

// `material` forms 3 * primitiveIndex (+ 0..2) and 3 * vertex (+ 0..2) in 32 bits: the positions surface_in_bounds proves inside
// (computed in 64 bits) are the ones it reads only if those products do not wrap
RDX_HD inline bool shade_triple_fits32(uint32_t item) { return item <= 0x55555554u; }      // 3 * item + 2 <= 0xffffffff

// a texture index of a Material: -1 (none) or a layer of the image array
RDX_HD inline bool shade_layer_in_bounds(int32_t texIdx, uint32_t layers) { return texIdx == -1 || (texIdx >= 0 && (uint32_t)texIdx < layers); }

// The bounds rule of rdx_shade_hits (include/rdx.h): may the closest-hit shader run on the record (instanceIndex, primitiveIndex)
// without a read outside a buffer?  Arguments up to `nuv` as surface_in_bounds; nuv = 0 when textures are off (the uv stream is
// not read then).  idx3 == null: the rule ends after the index range, which is what must hold before the indices MAY be read.
// With idx3 it goes on to the Material: materialIndex below nmaterials, and -- textures on -- each of the Material's four texture
// indices -1 or below `layers`.  `materials` is read only once materialIndex is known to be inside.
RDX_HD inline bool shade_in_bounds(const MeshInfo* table, uint32_t ninst, uint32_t nmeshinfo, uint32_t instanceIndex, uint32_t primitiveIndex,
                                   const uint32_t* idx3, uint64_t nindex, uint64_t nnormal, uint64_t nuv, const Material* materials,
                                   uint32_t nmaterials, bool textures, uint32_t layers)
{
    if (!shade_triple_fits32(primitiveIndex)) return false;
    if (!surface_in_bounds(table, ninst, nmeshinfo, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv)) return false;
    if (!idx3) return true;
    for (int k = 0; k < 3; ++k) if (!shade_triple_fits32(idx3[k])) return false;
    const int32_t m = table[instanceIndex].materialIndex;
    if (m < 0 || (uint32_t)m >= nmaterials) return false;
    if (!textures) return true;
    const Material& mt = materials[m];
    return shade_layer_in_bounds(mt.albedoTexIdx, layers) && shade_layer_in_bounds(mt.metallicTexIdx, layers) &&
           shade_layer_in_bounds(mt.roughnessTexIdx, layers) && shade_layer_in_bounds(mt.normalTexIdx, layers);
}

#if defined(__HIPCC__)
// rdx_shade_hits (shade.hip): n rays, their closest-hit query records and RNG keys in; one 48-byte shade record per ray out, and --
// each optional -- the next ray and the shadow ray of every surviving ray, packed when `src` is given.  *live += survivors,
// *invalid += records that fail shade_in_bounds.  All pointers are device pointers.
void launch_shade_hits(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const float4* rays, const float4* hits,
                       const uint4* keys, uint32_t n, const ShadeScene& sc, float4* shade, float4* next, float4* shadow, uint32_t* src,
                       uint32_t* live, uint32_t* invalid);
#endif

} // namespace rdx

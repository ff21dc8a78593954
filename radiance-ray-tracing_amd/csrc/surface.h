// surface.h -- what rdx_resolve_hits shares between the host runtime, its kernel (surface.hip) and the CPU tests: the view of the
// scene streams with their element counts, and the bounds rule of one hit record.  Compiles for host and device.
#pragma once
#include <stdint.h>

#include "rdx_types.h"

namespace rdx {

struct SurfaceScene {              // descriptor slots 5, 7, 8, 9 with their ELEMENT counts (MeshInfo records, indices, floats, floats)
    const MeshInfo* meshInfo;
    const uint32_t* index;
    const float* uv;               // null: u = v = 0 (nUv is 0 then)
    const float* normal;
    uint32_t nMeshInfo;
    uint64_t nIndex, nNormal, nUv;
};

// first + 2 < n for the three consecutive elements first, first + 1, first + 2 of a stream of n; offset is an int32 of a MeshInfo
// (it may be negative), `item` a 32-bit primitive or vertex number: the sum is exact in 64 bits (|offset| <= 2^31, 3 * item < 2^34)
RDX_HD inline bool surface_triple_in_bounds(int32_t offset, uint32_t item, uint64_t n)
{
    const int64_t first = (int64_t)offset + (int64_t)item * 3;
    return first >= 0 && (uint64_t)first + 2u < n;
}

// The bounds rule of rdx_resolve_hits (include/rdx.h): may the record (instanceIndex, primitiveIndex) be resolved without a read
// outside the streams?  `table` = the MeshInfo records (nmeshinfo of them); it is read only once instanceIndex is known to be
// inside.  idx3 = the triangle's three vertex numbers, or null when they have not been read yet: the rule then ends after the
// index range, which is what must hold before they MAY be read -- the kernel asks twice, before and after that gather.  nuv == 0
// (no uv stream) rejects nothing.
RDX_HD inline bool surface_in_bounds(const MeshInfo* table, uint32_t ninst, uint32_t nmeshinfo, uint32_t instanceIndex,
                                     uint32_t primitiveIndex, const uint32_t* idx3, uint64_t nindex, uint64_t nnormal, uint64_t nuv)
{
    if (instanceIndex >= ninst || instanceIndex >= nmeshinfo) return false;
    const MeshInfo& mi = table[instanceIndex];
    if (!surface_triple_in_bounds(mi.indexOffset, primitiveIndex, nindex)) return false;
    if (!idx3) return true;
    for (int k = 0; k < 3; ++k) {
        if (!surface_triple_in_bounds(mi.normalOffset, idx3[k], nnormal)) return false;
        // (u, v) are elements 0 and 1 of the vertex's triple
        if (nuv) { const int64_t first = (int64_t)mi.uvOffset + (int64_t)idx3[k] * 3; if (first < 0 || (uint64_t)first + 1u >= nuv) return false; }
    }
    return true;
}

} // namespace rdx

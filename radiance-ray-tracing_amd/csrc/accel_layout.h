// accel_layout.h -- derivation of the traversal layout (rdx_types.h "D*" structs) from a TLAS blob.
//
// Host arithmetic on a byte blob only: no device, no runtime context.  The runtime (rdx_runtime.cpp derive_accel) uploads the
// arrays and sizes the kernels' LDS from the need numbers; the test seam rdx_debug_accel_layout hands both to the CPU tests.
#pragma once
#include <stddef.h>
#include <stdint.h>

#include <string>
#include <vector>

#include "../../include/rdx.h"
#include "rdx_types.h"

namespace rdx {

constexpr uint32_t RDX_CULL_AUTO_MIN_WIDE = 1u << 20;      // option "cull" -1: scenes with at least this many inner BVH nodes take the culled walk

// the options the layout depends on (rdx_set_option "quad" / "cull": 1 on, 0 off, -1 automatic)
struct AccelOptions { int quad = 1; int cull = -1; };

struct AccelLayout {
    std::vector<DNode> tnodes;         // top-level nodes; w3 of a leaf: it holds a single-leaf BLAS of <= 8 triangles
    std::vector<DNode> ctnodes;        // the same nodes with the smaller-need child in the followed slot (cooperative kernel)
    std::vector<DInst> insts;
    std::vector<DNode> bnodes;         // BLAS nodes, merged: child / triangle indices are absolute
    std::vector<DTri> tris;
    std::vector<DWide> wide;           // one record per inner BLAS node, then the unified tree's records
    std::vector<DQuad> quad;           // index = DWide index; empty unless the exhaustive pool walk will use them
    uint32_t groupBits[9] = {};        // instance slots of the shared-transform group (bitmap of 8 words; the 9th stays 0)
    rdx_accel_scalars s{};             // need numbers and engine flags (include/rdx.h)
};

// 0, or -1 with the reason in `err`.  `out` is only meaningful after a 0.
int derive_accel_layout(const void* blob, size_t size, const AccelOptions& opt, AccelLayout& out, std::string& err);

} // namespace rdx

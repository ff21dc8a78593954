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

// Host-side bookkeeping of one derivation: where the block of every BLAS sits in the merged arrays and what the top-level steps
// need to know about it.  With it the top-level part of a layout can be derived again for other instance transforms without
// touching a BLAS node or triangle (update_accel_layout).
struct AccelBlasBlock {
    uint32_t relOffset;                // byte offset of the BLAS inside the blob's BLAS region (which starts behind the instance records)
    uint32_t nodeBase, triBase, nTris; // its blocks in bnodes / tris
    uint32_t need, coopNeed, anyNeed, quadNeed;      // stack needs of the engines inside this BLAS
    uint32_t coopPieces;               // what the cooperative kernel's stack needs on top of coopNeed: leaf pieces along a path
    uint32_t rootDesc0, rootDesc1;     // root of its wide records, as in DInst
    float rootMin[3], rootMax[3];
    uint32_t owner;                    // DTri._p0 of its triangles as the arrays stand: an instance slot, or 0xffffffff
    DQuad entry;                       // entry record of its root and the pool need of a walk from there (AccelLayout::entries)
    uint32_t entryNeed;
};
struct AccelBook {
    bool valid = false;                // false: the blob does not keep its BLASes behind the instance records (foreign blob)
    std::vector<AccelBlasBlock> blocks;
    uint64_t blasRegionBytes = 0;
    uint32_t nInst = 0, nTris = 0, nBlasWide = 0;    // nBlasWide: wide records of the BLAS blocks; the unified tree's follow
    uint32_t maxLeafChunks = 0, maxLeafTris = 0;
    bool hugeLeaf = false, coopBlasOK = true, quadBuilt = false;
};

struct AccelLayout {
    std::vector<DNode> tnodes;         // top-level nodes; w3 of a leaf: it holds a single-leaf BLAS of <= 8 triangles
    std::vector<DNode> ctnodes;        // the same nodes with the smaller-need child in the followed slot (cooperative kernel)
    std::vector<DInst> insts;
    std::vector<DNode> bnodes;         // BLAS nodes, merged: child / triangle indices are absolute
    std::vector<DTri> tris;
    std::vector<DWide> wide;           // one record per inner BLAS node, then the unified tree's records
    std::vector<DQuad> quad;           // index = DWide index; empty unless the exhaustive pool walk will use them
    std::vector<DQuad> entries;        // index = instance slot; empty unless `quad` is built.  Entry record of the instance's BLAS root R:
                                       // first half = the half quad_records() makes for a skipped child R (R's two children under
                                       // R's box, or R itself with its own box), second half empty; a leaf root has an inert record
    uint32_t entryNeed = 0;            // pool need of a walk that starts at an entry record (same recurrence as the quad records')
    uint32_t groupFirst = 0;           // lowest instance slot of the shared-transform group (0 without one)
    uint32_t groupBits[9] = {};        // instance slots of the shared-transform group (bitmap of 8 words; the 9th stays 0)
    rdx_accel_scalars s{};             // need numbers and engine flags (include/rdx.h)
    AccelBook book;
};

// 0, or -1 with the reason in `err`.  `out` is only meaningful after a 0.
int derive_accel_layout(const void* blob, size_t size, const AccelOptions& opt, AccelLayout& out, std::string& err);

// What update_accel_layout changed, for whoever keeps a copy of the arrays (the runtime: on a device).
struct AccelOwnerRange { uint32_t first, count, owner; };      // DTri._p0 = owner for triangle slots [first, first + count)
struct AccelUpdate {
    bool tnodes = false, ctnodes = false, insts = false, groupBits = false, entries = false;      // small arrays whose bytes changed
    std::vector<AccelOwnerRange> owners;
    uint32_t wideTailFirst = 0;        // the wide array is now [0, wideTailFirst) as before, then wideTail
    std::vector<DWide> wideTail;
    bool wideTailChanged = false;
};

// The layout of `blob` -- the blob `inout` was derived from with other transforms, SBT offsets or custom ids of its instances: same
// instance count, byte-identical BLAS region -- from the top-level steps alone.  The per-BLAS blocks of bnodes / tris / wide / quad
// stay where they are (a fresh derivation would order them by instance slot), so `inout` may come without those four arrays (the
// runtime drops them after the upload); tnodes, ctnodes, insts, groupBits, entries, the scalars and the book are replaced.  Triangle owner
// words and the tail of `wide` are only REPORTED in `what_changed`: apply_accel_update writes them into host arrays.
// 0 = done; 1 = this change needs the full derivation (quad records or the unified tree would appear or vanish, the blob does not
// match the book): `inout` is untouched; -1 = error, reason in `err`.
int update_accel_layout(const void* blob, size_t size, const AccelOptions& opt, AccelLayout& inout, AccelUpdate& what_changed, std::string& err);
// the reported owner words and wide tail, written into inout.tris / inout.wide (which must be present)
void apply_accel_update(AccelLayout& inout, const AccelUpdate& what_changed);

} // namespace rdx

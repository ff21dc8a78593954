// accel_layout.cpp -- the traversal layout of a TLAS blob (accel_layout.h): merged node / triangle arrays, wide records with
// normal cones, instance records, the shared-transform group, the unified tree, quad records and the stack needs of every
// engine.  Every exactness argument of DESIGN.md section 4 and docs/CULLED_WALK.md rests on what is written here.
#include "accel_layout.h"

#include <algorithm>
#include <array>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstring>
#include <functional>
#include <map>

#ifndef RDX_SBT_HEADER
#define RDX_SBT_HEADER "sbt_generated.h"      // tools/genSBT.py output (the table this library's stage kernels were built for)
#endif
#include RDX_SBT_HEADER

namespace rdx {
namespace {

// math.cl:56-183: cofactor inverse, term order preserved.  Returns false (out untouched) if det == 0.
bool inverse_mat4(const float* m, float* out)
{
    float inv[16];
    inv[0] = m[5] * m[10] * m[15] - m[5] * m[11] * m[14] - m[9] * m[6] * m[15] + m[9] * m[7] * m[14] + m[13] * m[6] * m[11] - m[13] * m[7] * m[10];
    inv[4] = -m[4] * m[10] * m[15] + m[4] * m[11] * m[14] + m[8] * m[6] * m[15] - m[8] * m[7] * m[14] - m[12] * m[6] * m[11] + m[12] * m[7] * m[10];
    inv[8] = m[4] * m[9] * m[15] - m[4] * m[11] * m[13] - m[8] * m[5] * m[15] + m[8] * m[7] * m[13] + m[12] * m[5] * m[11] - m[12] * m[7] * m[9];
    inv[12] = -m[4] * m[9] * m[14] + m[4] * m[10] * m[13] + m[8] * m[5] * m[14] - m[8] * m[6] * m[13] - m[12] * m[5] * m[10] + m[12] * m[6] * m[9];
    inv[1] = -m[1] * m[10] * m[15] + m[1] * m[11] * m[14] + m[9] * m[2] * m[15] - m[9] * m[3] * m[14] - m[13] * m[2] * m[11] + m[13] * m[3] * m[10];
    inv[5] = m[0] * m[10] * m[15] - m[0] * m[11] * m[14] - m[8] * m[2] * m[15] + m[8] * m[3] * m[14] + m[12] * m[2] * m[11] - m[12] * m[3] * m[10];
    inv[9] = -m[0] * m[9] * m[15] + m[0] * m[11] * m[13] + m[8] * m[1] * m[15] - m[8] * m[3] * m[13] - m[12] * m[1] * m[11] + m[12] * m[3] * m[9];
    inv[13] = m[0] * m[9] * m[14] - m[0] * m[10] * m[13] - m[8] * m[1] * m[14] + m[8] * m[2] * m[13] + m[12] * m[1] * m[10] - m[12] * m[2] * m[9];
    inv[2] = m[1] * m[6] * m[15] - m[1] * m[7] * m[14] - m[5] * m[2] * m[15] + m[5] * m[3] * m[14] + m[13] * m[2] * m[7] - m[13] * m[3] * m[6];
    inv[6] = -m[0] * m[6] * m[15] + m[0] * m[7] * m[14] + m[4] * m[2] * m[15] - m[4] * m[3] * m[14] - m[12] * m[2] * m[7] + m[12] * m[3] * m[6];
    inv[10] = m[0] * m[5] * m[15] - m[0] * m[7] * m[13] - m[4] * m[1] * m[15] + m[4] * m[3] * m[13] + m[12] * m[1] * m[7] - m[12] * m[3] * m[5];
    inv[14] = -m[0] * m[5] * m[14] + m[0] * m[6] * m[13] + m[4] * m[1] * m[14] - m[4] * m[2] * m[13] - m[12] * m[1] * m[6] + m[12] * m[2] * m[5];
    inv[3] = -m[1] * m[6] * m[11] + m[1] * m[7] * m[10] + m[5] * m[2] * m[11] - m[5] * m[3] * m[10] - m[9] * m[2] * m[7] + m[9] * m[3] * m[6];
    inv[7] = m[0] * m[6] * m[11] - m[0] * m[7] * m[10] - m[4] * m[2] * m[11] + m[4] * m[3] * m[10] + m[8] * m[2] * m[7] - m[8] * m[3] * m[6];
    inv[11] = -m[0] * m[5] * m[11] + m[0] * m[7] * m[9] + m[4] * m[1] * m[11] - m[4] * m[3] * m[9] - m[8] * m[1] * m[7] + m[8] * m[3] * m[5];
    inv[15] = m[0] * m[5] * m[10] - m[0] * m[6] * m[9] - m[4] * m[1] * m[10] + m[4] * m[2] * m[9] + m[8] * m[1] * m[6] - m[8] * m[2] * m[5];
    float det = m[0] * inv[0] + m[1] * inv[4] + m[2] * inv[8] + m[3] * inv[12];
    if (det == 0) return false;
    det = 1.0f / det;
    for (int i = 0; i < 16; ++i) out[i] = inv[i] * det;
    return true;
}

// worst-case stack occupancy of the left-first DFS in kernels.hip (right child pushed, left followed)
uint32_t blas_need(const BlobNode* nodes, uint32_t idx)
{
    // iterative post-order to survive deep trees
    struct Frame { uint32_t idx; uint32_t needL; int state; };
    std::vector<Frame> st{{idx, 0, 0}};
    uint32_t ret = 0;
    while (!st.empty()) {
        Frame& f = st.back();
        const BlobNode& n = nodes[f.idx];
        if (n.w0 & LEAF_BIT) { ret = 0; st.pop_back(); continue; }
        if (f.state == 0) { f.state = 1; st.push_back({n.w0, 0, 0}); continue; }
        if (f.state == 1) { f.needL = ret; f.state = 2; st.push_back({n.w1, 0, 0}); continue; }
        ret = std::max(1u + f.needL, ret);
        st.pop_back();
    }
    return ret;
}

// Cone of lines around the normals of a set of triangles + their worst shape; see DESIGN.md 4.1c for what the culled walk
// proves from it.  kappa0 = 2^-7: the culled walk skips a subtree / a leaf only for rays that make at least asin(kappa0 / q)
// with the plane of every triangle below the node.
struct NormalCone {
    double a[3] = {0, 0, 0};       // axis (unit) -- valid when n > 0
    double alpha = 0;              // half-angle: every normal line is within alpha of the axis line
    double q = 1;                  // min over the triangles of sin(angle(e1, e2))
    bool never = false;            // degenerate triangle, or the normals do not fit a cone of < 90 degrees
    uint32_t n = 0;
    static double ang(const double* x, const double* y)      // angle between two LINES
    {
        const double c = std::fabs(x[0] * y[0] + x[1] * y[1] + x[2] * y[2]);
        return std::acos(std::min(1.0, c));
    }
    void add_normal(const double* nn, double a1)
    {
        if (n == 0) { a[0] = nn[0]; a[1] = nn[1]; a[2] = nn[2]; alpha = a1; n = 1; return; }
        NormalCone o; o.a[0] = nn[0]; o.a[1] = nn[1]; o.a[2] = nn[2]; o.alpha = a1; o.n = 1;
        merge(o);
    }
    void add_triangle(const DTri& t)
    {
        const double e1[3] = {t.e1[0], t.e1[1], t.e1[2]}, e2[3] = {t.e2[0], t.e2[1], t.e2[2]};
        const double c[3] = {e1[1] * e2[2] - e1[2] * e2[1], e1[2] * e2[0] - e1[0] * e2[2], e1[0] * e2[1] - e1[1] * e2[0]};
        const double lc = std::sqrt(c[0] * c[0] + c[1] * c[1] + c[2] * c[2]);
        const double l1 = std::sqrt(e1[0] * e1[0] + e1[1] * e1[1] + e1[2] * e1[2]), l2 = std::sqrt(e2[0] * e2[0] + e2[1] * e2[1] + e2[2] * e2[2]);
        if (!(lc > 0) || !(l1 > 0) || !(l2 > 0) || !std::isfinite(lc) || !std::isfinite(l1 * l2)) { never = true; return; }
        q = std::min(q, lc / (l1 * l2));
        const double nn[3] = {c[0] / lc, c[1] / lc, c[2] / lc};
        add_normal(nn, 0.0);
    }
    void merge(const NormalCone& o)
    {
        never = never || o.never; q = std::min(q, o.q);
        if (o.n == 0) return;
        if (n == 0) { a[0] = o.a[0]; a[1] = o.a[1]; a[2] = o.a[2]; alpha = o.alpha; n = o.n; return; }
        const double sgn = (a[0] * o.a[0] + a[1] * o.a[1] + a[2] * o.a[2]) < 0 ? -1.0 : 1.0;
        const double gam = ang(a, o.a);
        n += o.n;
        if (gam + o.alpha <= alpha) return;                                        // o inside this cone
        if (gam + alpha <= o.alpha) { a[0] = o.a[0]; a[1] = o.a[1]; a[2] = o.a[2]; alpha = o.alpha; return; }
        // smallest cone around both: axis between the two, rotated from a towards o by (gam + o.alpha - alpha) / 2
        const double na = (gam + alpha + o.alpha) / 2;
        const double w = gam > 1e-12 ? (na - alpha) / gam : 0.5;
        double m[3] = {a[0] * (1 - w) + sgn * o.a[0] * w, a[1] * (1 - w) + sgn * o.a[1] * w, a[2] * (1 - w) + sgn * o.a[2] * w};
        const double lm = std::sqrt(m[0] * m[0] + m[1] * m[1] + m[2] * m[2]);
        if (!(lm > 1e-9)) { never = true; return; }
        for (int k = 0; k < 3; ++k) m[k] /= lm;
        // (the linear blend is not the exact bisecting rotation: take the half-angle from the blended axis itself)
        const double sgn_o[3] = {sgn * o.a[0], sgn * o.a[1], sgn * o.a[2]};
        alpha = std::max(ang(m, a) + alpha, ang(m, sgn_o) + o.alpha);
        a[0] = m[0]; a[1] = m[1]; a[2] = m[2];
    }
    // x | y << 8 | z << 16 | T << 24 (T: 7 bits, rdx_types.h wide_desc): a ray may be culled against this leaf / subtree only if
    // |d^ . a'| >= T / 127 with a' = (b - 127.5) / 127 the quantised axis.  Derivation: every normal line is within
    // alpha + eq of a' (eq: quantisation), so the ray makes >= asin|d^ . a'^| - (alpha + eq) with every triangle's plane; that must be
    // >= asin(kappa0 / q).  |a'| is within 0.7 % of 1, which the factor 1.0075 covers, fp32 evaluation another 1e-5.
    uint32_t pack() const
    {
        const double kappa0 = 1.0 / 128.0, eq = 0.0085;
        uint32_t T = WIDE_CONE_NEVER;
        uint32_t b[3] = {128, 128, 128};
        if (!never && n > 0 && q > kappa0 && alpha + eq < 1.5) {
            const double need = std::asin(std::min(1.0, kappa0 / q)) + alpha + eq;     // angle the ray must make with the axis PLANE
            if (need < 1.55) {
                const double thr = std::sin(need) * 1.0075 * 1.00002;
                const double t8 = std::ceil(thr * 127.0) + 1.0;
                if (t8 <= 126.0) T = (uint32_t)t8;
            }
            for (int k = 0; k < 3; ++k) b[k] = (uint32_t)std::min(255.0, std::max(0.0, std::floor(127.5 + 127.0 * a[k] + 0.5)));
        }
        return b[0] | (b[1] << 8) | (b[2] << 16) | (T << 24);
    }
};

// Can the order-free engines (pool / cooperative / per-lane wide) trace instances whose SBT offset is k?  They assume that a
// radiance ray's row (1 + k) has NO any-hit shader -- so the winner is the minimum, whatever the visiting order -- and that a
// shadow ray's row (2 + k) is the stock pair: an any-hit shader that ends the walk at the first accepted candidate and a
// closest-hit shader that only flags the hit (`anyShadow` / `shadow`: neither looks at WHICH candidate it was).  Rows are those
// of the sbt.json this library was generated from (tools/genSBT.py -> sbt_generated.h); k = 0 always qualifies for the stock
// table.  Anything else keeps the reference's DFS order: the reference-order kernel.
bool sbt_offset_is_order_free(uint32_t k)
{
    struct Row { int row; const char* fn; };
    static const Row anyHit[] = {
#define X(row, fn) {row, #fn},
        RDX_SBT_ANY_HIT(X)
#undef X
        {-1, nullptr}};
    static const Row closest[] = {
#define X(row, fn) {row, #fn},
        RDX_SBT_CLOSEST_HIT(X)
#undef X
        {-1, nullptr}};
    auto find = [](const Row* t, int row) -> const char* { for (; t->fn; ++t) if (t->row == row) return t->fn; return nullptr; };
    if (k > 1000000u) return false;
    const int r1 = 1 + (int)k, r2 = 2 + (int)k;
    if (find(anyHit, r1)) return false;
    const char* a2 = find(anyHit, r2); const char* c2 = find(closest, r2);
    const char* a0 = find(anyHit, 2); const char* c0 = find(closest, 2);
    auto same = [](const char* x, const char* y) { return (x == nullptr && y == nullptr) || (x && y && !std::strcmp(x, y)); };
    return same(a2, a0) && same(c2, c0);
}

bool is_identity(const float* m)      // (zero signs do not matter)
{
    for (int e = 0; e < 16; ++e) if (!(m[e] == ((e % 5 == 0) ? 1.0f : 0.0f))) return false;
    return true;
}

// Entry order of a quad record, arrangement arr = 0..7: ord[j] = which of the four entries (0, 1: half of child 0; 2, 3: half of
// child 1) is stored at position j.  Bit 0 swaps the halves, bits 1 / 2 swap the entries inside the first / second stored half.
void quad_order(int arr, int ord[4])
{
    const int h0 = (arr & 1) ? 2 : 0, h1 = (arr & 1) ? 0 : 2;
    ord[0] = h0 + ((arr >> 1) & 1); ord[1] = h0 + 1 - ((arr >> 1) & 1);
    ord[2] = h1 + ((arr >> 2) & 1); ord[3] = h1 + 1 - ((arr >> 2) & 1);
}

struct BlasInfo { uint32_t nodeBase; uint32_t need; uint32_t coopNeed; uint32_t coopPieces; uint32_t anyNeed; uint32_t triBase; uint32_t rootDesc0, rootDesc1; float rootMin[3], rootMax[3];
                  uint32_t nTris; uint32_t users;
                  uint32_t quadNeed;        // pool-stack need of the quad walk from its root (0: leaf root, or no quad records)
                  uint32_t owner;           // DTri._p0 of its triangles: the slot of its one instance (group / unified tree), or 0xffffffff
                  DQuad entry;              // entry record of its root (step 6b) and the pool need of a walk that starts there;
                  uint32_t entryNeed; };    // need 0 and an inert record: leaf root, or no quad records

// one derivation: the steps below run in the order of derive_accel_layout and share this state
struct Deriver {
    const uint8_t* blob; size_t bsz;
    AccelOptions opt;
    AccelLayout& L;
    std::string& err;
    // step 1
    uint32_t nTop = 0, nInst = 0;
    const BlobNode* tnodes = nullptr;
    const BlobInst* binst = nullptr;
    // steps 2, 3
    std::map<uint32_t, BlasInfo> blasAt;    // byte offset -> merged-array base
    bool hugeLeaf = false;                  // a leaf of more triangles than the wide layout's count field holds
    bool coopOK = true, coopBlasOK = true;
    bool sbtOffsets = false;
    uint32_t maxLeafChunks = 0;             // extra stack entries an oversized (> 8 triangle) leaf can push
    uint32_t maxLeafTris = 0;
    // step 6
    std::vector<uint32_t> qneed;
    uint32_t unifiedQuadNeed = 0;
    // update_accel_layout: L holds no BLAS blocks -- blasAt comes from the book, L.wide is only the tail behind wideOffset records
    bool update = false, needFull = false;
    uint32_t wideOffset = 0, bookTris = 0;
    uint32_t nBlasWide = 0;                 // wide records of the BLAS blocks (the unified tree's follow)
    uint32_t total_tris() const { return update ? bookTris : (uint32_t)L.tris.size(); }
    uint32_t total_wide() const { return wideOffset + (uint32_t)L.wide.size(); }
    bool want_quad() const
    {
        return opt.quad != 0 && !(opt.cull > 0 || (opt.cull < 0 && total_wide() >= RDX_CULL_AUTO_MIN_WIDE)) && !L.s.unifiedRoot;
    }

    int fail(const char* fmt, ...)
    {
        va_list ap, ap2; va_start(ap, fmt); va_copy(ap2, ap);
        const int n = vsnprintf(nullptr, 0, fmt, ap); va_end(ap);
        err.assign((size_t)(n > 0 ? n : 0) + 1, '\0');
        vsnprintf(&err[0], err.size(), fmt, ap2); va_end(ap2);
        err.resize((size_t)(n > 0 ? n : 0));
        return -1;
    }

    int import_top();
    int import_blas(uint32_t byteOffset, BlasInfo& info);
    int blas_wide_records(const BlobNode* bn, uint32_t nNodes, uint32_t triBase, BlasInfo& info);
    int instance_records();
    void world_box(const BlobInst& bi, DInst& d);
    void shared_transform_group();
    void unified_tree();
    void write_owners();
    int quad_records();
    void entry_records();
    void make_book();
    int top_level_needs();
};

// ---- step 1: validate and import the top level -------------------------------------------------------------------------------
int Deriver::import_top()
{
    if (bsz < 16) return fail("TLAS buffer too small");
    const auto* th = reinterpret_cast<const BlobTopHeader*>(blob);
    if (th->type != TYPE_TOP_AS || th->nodeByteOffset != 16 || th->instByteOffset < 16 + sizeof(BlobNode) ||
        th->instByteOffset > bsz || th->totalBufferSize > bsz)
        return fail("descriptor slot 13 does not hold a top-level acceleration structure blob");
    nTop = (th->instByteOffset - th->nodeByteOffset) / sizeof(BlobNode);
    tnodes = reinterpret_cast<const BlobNode*>(blob + th->nodeByteOffset);
    binst = reinterpret_cast<const BlobInst*>(blob + th->instByteOffset);
    // instance count = max leaf (start+count)
    for (uint32_t i = 0; i < nTop; ++i)
        if (tnodes[i].w0 & LEAF_BIT) nInst = std::max(nInst, tnodes[i].w1 + (tnodes[i].w0 & 0x7fffffffu));
    if ((size_t)th->instByteOffset + (size_t)nInst * sizeof(BlobInst) > bsz) return fail("TLAS blob: instance array out of range");

    // The derived layout (stack needs computed children-first, first-in-DFS tie-break = lowest slot) relies on the numbering
    // the reference's flattener produces (bvh.cpp:475-497,551-563): DFS pre-order -- left child = parent + 1, right child
    // behind the whole left subtree -- and leaves listing their instances / triangles in leaf order.  A foreign or
    // corrupted blob (e.g. a cache file without side-car) that breaks it is refused here rather than mis-sized on the GPU.
    std::vector<DNode>& dT = L.tnodes;
    dT.resize(nTop);
    uint32_t expectInst = 0;
    for (uint32_t i = 0; i < nTop; ++i) {
        std::memcpy(&dT[i], &tnodes[i], sizeof(BlobNode));
        if (!(tnodes[i].w0 & LEAF_BIT)) {
            if (tnodes[i].w0 >= nTop || tnodes[i].w1 >= nTop) return fail("TLAS blob: child index out of range");
            if (tnodes[i].w0 != i + 1 || tnodes[i].w1 <= tnodes[i].w0) return fail("TLAS blob: node %u is not in DFS pre-order (children %u, %u)", i, tnodes[i].w0, tnodes[i].w1);
        } else {
            if (tnodes[i].w1 != expectInst) return fail("TLAS blob: leaf %u does not list its instances in leaf order (start %u, expected %u)", i, tnodes[i].w1, expectInst);
            expectInst += tnodes[i].w0 & 0x7fffffffu;
        }
    }
    coopOK = nInst <= RDX_COOP_MAX_INSTANCES;
    return 0;
}

// ---- step 2: import one BLAS -------------------------------------------------------------------------------------------------
// nodes and triangles into the merged arrays (indices made absolute), then its wide records
int Deriver::import_blas(uint32_t byteOffset, BlasInfo& info)
{
    std::vector<DNode>& dB = L.bnodes;
    std::vector<DTri>& dTri = L.tris;
    if ((size_t)byteOffset + 16 > bsz) return fail("TLAS blob: BLAS offset out of range");
    const uint8_t* bb = blob + byteOffset;
    const auto* bh = reinterpret_cast<const BlobBotHeader*>(bb);
    if (bh->type != TYPE_BOT_AS || bh->faceByteOffset < bh->nodeByteOffset || bh->vertexOffset < bh->faceByteOffset ||
        (size_t)byteOffset + bh->vertexOffset > bsz)
        return fail("TLAS blob: malformed bottom-level structure at byte %u", byteOffset);
    const uint32_t nNodes = (bh->faceByteOffset - bh->nodeByteOffset) / sizeof(BlobNode);
    const uint32_t nTris = (bh->vertexOffset - bh->faceByteOffset) / sizeof(BlobTri);
    const auto* bn = reinterpret_cast<const BlobNode*>(bb + bh->nodeByteOffset);
    const auto* bt = reinterpret_cast<const BlobTri*>(bb + bh->faceByteOffset);
    const auto* bv = reinterpret_cast<const float*>(bb + bh->vertexOffset);
    const size_t vertFloatsAvail = (bsz - byteOffset - bh->vertexOffset) / 4;
    const uint32_t nodeBase = (uint32_t)dB.size(), triBase = (uint32_t)dTri.size();
    if ((uint64_t)nodeBase + nNodes >= (1u << 30)) return fail("too many BVH nodes for 30-bit references");
    dB.resize(nodeBase + nNodes);
    uint32_t expectTri = 0;
    for (uint32_t i = 0; i < nNodes; ++i) {
        DNode& d = dB[nodeBase + i];
        std::memcpy(&d, &bn[i], sizeof(BlobNode));
        if (bn[i].w0 & LEAF_BIT) {
            if ((uint64_t)bn[i].w1 + (bn[i].w0 & 0x7fffffffu) > nTris) return fail("BLAS blob: leaf range out of bounds");
            if (bn[i].w2 == TYPE_TRIG) {
                if (bn[i].w1 != expectTri) return fail("BLAS blob: leaf %u does not list its triangles in leaf order (start %u, expected %u)", i, bn[i].w1, expectTri);
                expectTri += bn[i].w0 & 0x7fffffffu;
            }
            maxLeafChunks = std::max(maxLeafChunks, 2u * (((bn[i].w0 & 0x7fffffffu) + 7u) / 8u));
            maxLeafTris = std::max(maxLeafTris, bn[i].w0 & 0x7fffffffu);
            d.w1 = bn[i].w1 + triBase;
        } else {
            if (bn[i].w0 >= nNodes || bn[i].w1 >= nNodes) return fail("BLAS blob: child index out of range");
            if (bn[i].w0 != i + 1 || bn[i].w1 <= bn[i].w0) return fail("BLAS blob: node %u is not in DFS pre-order (children %u, %u)", i, bn[i].w0, bn[i].w1);
            d.w0 = bn[i].w0 + nodeBase; d.w1 = bn[i].w1 + nodeBase;
        }
    }
    if ((uint64_t)triBase + nTris > LEAF_START_MASK) return fail("too many triangles for 27-bit triangle-run references");
    dTri.resize(triBase + nTris);
    for (uint32_t i = 0; i < nTris; ++i) {
        const BlobTri& t = bt[i];
        if ((size_t)std::max({t.idx0, t.idx1, t.idx2}) * 4 + 3 > vertFloatsAvail)
            return fail("BLAS blob: vertex index out of range");
        const float* v0 = bv + 4 * (size_t)t.idx0; const float* v1 = bv + 4 * (size_t)t.idx1; const float* v2 = bv + 4 * (size_t)t.idx2;
        DTri& d = dTri[triBase + i];
        d.v0[0] = v0[0]; d.v0[1] = v0[1]; d.v0[2] = v0[2]; d.primID = t.primID;
        d.e1[0] = v1[0] - v0[0]; d.e1[1] = v1[1] - v0[1]; d.e1[2] = v1[2] - v0[2]; d._p0 = 0xffffffffu;   // radiance.cl:215; _p0: see "shared-transform group"
        d.e2[0] = v2[0] - v0[0]; d.e2[1] = v2[1] - v0[1]; d.e2[2] = v2[2] - v0[2]; d._p1 = triBase;       // radiance.cl:216; _p1: first triangle slot of this BLAS
    }
    info = BlasInfo{};
    for (int hh = 0; hh < 2; ++hh) { info.entry.half[hh].ld1 = WIDE_LEAF; info.entry.half[hh].rd1 = WIDE_LEAF; }
    info.nodeBase = nodeBase; info.triBase = triBase; info.nTris = nTris; info.users = 0; info.owner = 0xffffffffu;
    if (blas_wide_records(bn, nNodes, triBase, info)) return -1;
    if (nTris > RDX_COOP_MAX_BLAS_TRIS) { coopOK = false; coopBlasOK = false; }
    for (int k = 0; k < 3; ++k) { info.rootMin[k] = bn[0].bottom[k]; info.rootMax[k] = bn[0].top[k]; }
    return 0;
}

// wide layout of one BLAS: one record per inner node, numbered in the same DFS pre-order; the normal cones of its children;
// the stack needs of the BLAS for every engine; its root descriptor
int Deriver::blas_wide_records(const BlobNode* bn, uint32_t nNodes, uint32_t triBase, BlasInfo& info)
{
    std::vector<DTri>& dTri = L.tris;
    std::vector<DWide>& dW = L.wide;
    const uint32_t wideBase = (uint32_t)dW.size();
    std::vector<uint32_t> wideIdx(nNodes, 0);
    uint32_t nInner = 0;
    for (uint32_t i = 0; i < nNodes; ++i) if (!(bn[i].w0 & LEAF_BIT)) wideIdx[i] = nInner++;
    if ((uint64_t)wideBase + nInner >= (1u << 30)) return fail("too many BVH nodes for 30-bit references");
    std::vector<NormalCone> cone(nNodes);
    auto desc = [&](uint32_t c, uint32_t& d0, uint32_t& d1) {
        if (bn[c].w0 & LEAF_BIT) {
            const uint32_t cnt = bn[c].w2 == TYPE_TRIG ? (bn[c].w0 & 0x7fffffffu) : 0u;
            if (cnt > WIDE_MAX_LEAF_TRIS) hugeLeaf = true;
            wide_desc(true, bn[c].w1 + triBase, std::min(cnt, (uint32_t)WIDE_MAX_LEAF_TRIS), cone[c].pack(), d0, d1);
        } else wide_desc(false, wideBase + wideIdx[c], 0u, cone[c].pack(), d0, d1);
    };
    dW.resize(wideBase + nInner);
    // Normal cones (culled walk, kernels.hip): for every node the cone of LINES that holds the normals of all triangles
    // below it -- axis, half-angle alpha -- and the worst triangle shape q = min sin(angle(e1, e2)).  Bottom-up (children
    // have larger indices); computed in double from the fp32 edge vectors the intersection test uses.
    for (uint32_t i = nNodes; i-- > 0;) {
        NormalCone& c = cone[i];
        if (bn[i].w0 & LEAF_BIT) {
            const uint32_t cnt = bn[i].w2 == TYPE_TRIG ? (bn[i].w0 & 0x7fffffffu) : 0u;
            for (uint32_t t = 0; t < cnt; ++t) c.add_triangle(dTri[triBase + bn[i].w1 + t]);
        } else { c = cone[bn[i].w0]; c.merge(cone[bn[i].w1]); }
    }
    // Stack need of the wide walk: a leaf child is queued, never pushed; of two inner children one is followed
    // and the other pushed.  The visiting order is free, so the child with the SMALLER need goes
    // into the "followed" (left) half of the record: need = max(1 + smaller, larger) instead of
    // max(1 + left, right).  Children have larger indices than their parent (DFS pre-order).
    std::vector<uint32_t> aneed(nNodes, 0);                     // any push order: 1 + the deeper inner child
    std::vector<uint32_t> cneed(nNodes, 0), wneed(nNodes, 0);   // wneed: per-lane wide kernel on the same records (pushes leaves too)
    std::vector<uint32_t> pneed(nNodes, 0);                     // cneed + the leaf pieces the cooperative kernel stacks
    auto leaf_pieces = [](const BlobNode& n) {                  // stack entries of a leaf child: all but its last 8-triangle piece
        const uint32_t cnt = n.w2 == TYPE_TRIG ? std::min(n.w0 & 0x7fffffffu, (uint32_t)WIDE_MAX_LEAF_TRIS) : 0u;
        return cnt ? (cnt - 1u) / 8u : 0u;
    };
    for (uint32_t i = nNodes; i-- > 0;) {
        if (bn[i].w0 & LEAF_BIT) continue;
        uint32_t a = bn[i].w0, b = bn[i].w1;
        const bool la = bn[a].w0 & LEAF_BIT, lb = bn[b].w0 & LEAF_BIT;
        if (!la && !lb) {
            aneed[i] = 1u + std::max(aneed[a], aneed[b]);
            if (cneed[b] < cneed[a]) std::swap(a, b);
            cneed[i] = std::max(1u + cneed[a], cneed[b]);
        } else {
            cneed[i] = la ? (lb ? 0u : cneed[b]) : cneed[a];
            aneed[i] = la ? (lb ? 0u : aneed[b]) : aneed[a];
        }
        // Kernels that keep a lane's work on a stack (per-lane wide kernel, cooperative kernel) put all but the last 8-triangle
        // piece of an oversized leaf child there, and those entries stay while the record's other child is walked: the pieces
        // of every oversized leaf along a path are on the stack together, so they are part of the recurrence.  (The pool
        // engine queues leaf triangles and keeps no such entries: cneed / aneed stay free of them.)
        const uint32_t pieces = (la ? leaf_pieces(bn[a]) : 0u) + (lb ? leaf_pieces(bn[b]) : 0u);
        wneed[i] = pieces + std::max(1u + wneed[a], wneed[b]);
        pneed[i] = pieces + ((!la && !lb) ? std::max(1u + pneed[a], pneed[b]) : (la ? (lb ? 0u : pneed[b]) : pneed[a]));
        DWide& w = dW[wideBase + wideIdx[i]];
        const BlobNode& Ln = bn[a]; const BlobNode& Rn = bn[b];
        for (int k = 0; k < 3; ++k) { w.lmin[k] = Ln.bottom[k]; w.lmax[k] = Ln.top[k]; w.rmin[k] = Rn.bottom[k]; w.rmax[k] = Rn.top[k]; }
        desc(a, w.ld0, w.ld1);
        desc(b, w.rd0, w.rd1);
    }
    info.need = std::max(blas_need(bn, 0), wneed[0]); info.coopNeed = cneed[0]; info.anyNeed = aneed[0];
    info.coopPieces = pneed[0] - cneed[0];
    desc(0, info.rootDesc0, info.rootDesc1);
    return 0;
}

// ---- step 3: instance records and world boxes --------------------------------------------------------------------------------
int Deriver::instance_records()
{
    std::vector<DInst>& dI = L.insts;
    dI.resize(nInst);
    for (uint32_t k = 0; k < nInst; ++k) {
        const BlobInst& bi = binst[k];
        // Dispatch index = instanceSBTOffset + sbtRecordOffset (radiance.cl:281, shader.cl:574-605).  With a non-zero offset the
        // any-hit shader of a RADIANCE ray's row may end the walk at the first accepted candidate in the reference's DFS order --
        // an order only the reference-order kernel keeps -- so scenes with such a row are traced by that kernel; offsets whose
        // rows behave like the stock rows 1 / 2 (sbt_offset_is_order_free) stay on the production engines (the live loader always
        // writes 0, tools/sceneBuilder.cpp:302).
        if (bi.SBTOffset != 0 && !sbt_offset_is_order_free(bi.SBTOffset)) sbtOffsets = true;
        auto it = blasAt.find(bi.instanceOffset);
        if (it == blasAt.end()) {
            if (update) { needFull = true; return -1; }      // a BLAS the book does not know
            BlasInfo info;
            if (import_blas(bi.instanceOffset, info)) return -1;
            it = blasAt.emplace(bi.instanceOffset, info).first;
        }
        it->second.users++;
        DInst& d = dI[k];
        std::memset(&d, 0, sizeof d);
        std::memcpy(d.fwd, bi.m, 64);
        inverse_mat4(bi.m, d.inv);          // zeros stay if singular (oracle convention; reference: uninitialised)
        d.SBTOffset = bi.SBTOffset; d.instanceID = bi.instanceID; d.customInstanceID = bi.customInstanceID;
        d.blasRoot = it->second.nodeBase;
        d.rootDesc0 = it->second.rootDesc0; d.rootDesc1 = it->second.rootDesc1; d._p0 = it->second.triBase;
        for (int c = 0; c < 3; ++c) { d.rootMin[c] = it->second.rootMin[c]; d.rootMax[c] = it->second.rootMax[c]; }
        world_box(bi, d);
    }
    return 0;
}

// conservative world-space box of the root OBB + margin coefficient for the instance pre-test
void Deriver::world_box(const BlobInst& bi, DInst& d)
{
    double lo[3] = {1e300, 1e300, 1e300}, hi[3] = {-1e300, -1e300, -1e300}, fa = 0, fi = 0;
    bool finite = true;
    for (int c = 0; c < 8; ++c) {
        const double p[3] = {(c & 1) ? d.rootMax[0] : d.rootMin[0], (c & 2) ? d.rootMax[1] : d.rootMin[1], (c & 4) ? d.rootMax[2] : d.rootMin[2]};
        for (int r = 0; r < 3; ++r) {
            const double w = (double)bi.m[4 * r] * p[0] + (double)bi.m[4 * r + 1] * p[1] + (double)bi.m[4 * r + 2] * p[2] + (double)bi.m[4 * r + 3];
            lo[r] = std::min(lo[r], w); hi[r] = std::max(hi[r], w);
            finite = finite && std::isfinite(w);
        }
    }
    for (int r = 0; r < 3; ++r) for (int c = 0; c < 3; ++c) { fa += (double)bi.m[4 * r + c] * bi.m[4 * r + c]; fi += (double)d.inv[4 * r + c] * d.inv[4 * r + c]; }
    const bool affine = bi.m[12] == 0.f && bi.m[13] == 0.f && bi.m[14] == 0.f && bi.m[15] == 1.f;
    const double kappa = std::sqrt(fa) * std::sqrt(fi);
    const bool usable = finite && affine && !(d.rootDesc1 & WIDE_LEAF) && kappa > 0 && kappa < 1e4 && std::isfinite(kappa);
    double ext = 0;
    for (int r = 0; r < 3; ++r) {
        d.worldMin[r] = std::nextafterf((float)lo[r], -INFINITY); d.worldMax[r] = std::nextafterf((float)hi[r], INFINITY);
        ext = std::max(ext, std::max(std::fabs(lo[r]), std::fabs(hi[r])));
    }
    // margin = c * (|o|_inf + ext): 64 x the first-order bound 4u*kappa on the displacement of the
    // object-space ray the reference builds in fp32 (DESIGN.md "instance pre-test")
    d.worldMin[3] = usable ? (float)(64.0 * 5.97e-8 * 4.0 * kappa) : -1.0f;
    d.worldMax[3] = (float)ext;
}

// ---- step 4: shared-transform group ------------------------------------------------------------------------------------------
// Shared-transform group (pool engine, flat top level).  The object-space ray of an instance is inverse(object->world) applied
// to the world ray with the reference's expressions (radiance.cl:161-169) -- a function of the inverse matrix's BITS and the
// ray alone.  Instances whose inverse matrices are bit-identical (a loader that puts every mesh of an OBJ under one node:
// all identity, tools/sceneBuilder.cpp:287-315; every scene of this repository's bench) therefore share ONE object-space
// ray: a wave lane writes it to its LDS ray slot once and enters all of them without waiting for one instance's subtree and
// queued tests to drain before the next (traverse_pool.h).  The instance slot a candidate belongs to then cannot come from
// the ray slot; it is kept in the triangle record (DTri._p0), which needs the BLAS to belong to exactly one instance.
// The largest such set of instances (>= 2, inner-node roots only) is the group.
void Deriver::shared_transform_group()
{
    std::vector<DInst>& dI = L.insts;
    if (nInst > 256) return;
    std::map<std::array<uint32_t, 16>, std::vector<uint32_t>> byInv;
    for (uint32_t k = 0; k < nInst; ++k) {
        const BlasInfo& bi = blasAt[binst[k].instanceOffset];
        if (bi.users != 1 || (dI[k].rootDesc1 & WIDE_LEAF)) continue;
        std::array<uint32_t, 16> key;
        std::memcpy(key.data(), dI[k].inv, 64);
        byInv[key].push_back(k);
    }
    const std::vector<uint32_t>* best = nullptr;
    for (auto& kv : byInv) if (kv.second.size() >= 2 && (!best || kv.second.size() > best->size())) best = &kv.second;
    if (!best) return;
    // identity group: the group's object-space ray equals the world ray up to the sign of zeros, on which no slab decision
    // depends -- the flat top-level step then runs the reference's root-box test of these instances itself (world ray)
    L.s.groupIdentity = is_identity(dI[(*best)[0]].inv);
    for (uint32_t k : *best) {
        L.groupBits[k >> 5] |= 1u << (k & 31u); ++L.s.groupCount;
        blasAt[binst[k].instanceOffset].owner = k;
    }
}

// ---- step 5: unified tree ----------------------------------------------------------------------------------------------------
// Unified tree (pool engine; scenes whose top level is too large for the flat step: > 64 nodes or > 256 instances -- a loader
// that makes one instance per mesh, tools/sceneBuilder.cpp:287-315).  When EVERY instance has the identity transform and a
// BLAS of its own, the object-space ray of all instances is one ray (the group's; it equals the world ray up to the sign
// of zeros, which no slab decision depends on: (b - o) / d keeps its value, min / max of +-0 or of equally signed infinities
// decide the same) -- so top-level nodes can be walked like BLAS nodes, by the pool, on that one ray slot:
//   top-level inner node -> wide record (boxes of its two children; an inner child is entered iff its box is hit, as the
//                           reference does when it pops the child; a leaf child is always entered: the reference never tests it)
//   top-level leaf       -> a balanced fan-out of always-entered pseudo nodes over its instances
//   instance             -> a child entry whose box is the BLAS root box and whose descriptor is the BLAS root (the root
//                           test of radiance.cl:61-63 for an inner root; a leaf root has its triangles tested directly)
// One item -- a super-root that holds the top-level root's box -- starts a ray; no top-level step, no instance step.
void Deriver::unified_tree()
{
    std::vector<DInst>& dI = L.insts;
    std::vector<DWide>& dW = L.wide;      // (update: only the tail, behind wideOffset records)
    if (!((nTop > 64 || nInst > 256) && nInst >= 2 && !(tnodes[0].w0 & LEAF_BIT) && !sbtOffsets)) return;
    for (uint32_t k = 0; k < nInst; ++k) {
        if (blasAt[binst[k].instanceOffset].users != 1) return;
        if (!is_identity(dI[k].inv)) return;
        if (std::memcmp(dI[k].inv, dI[0].inv, 64) != 0) return;                                               // ... but one ray needs one matrix
    }
    const float BIG = 1.0e30f;
    const uint32_t never = WIDE_CONE_NEVER << 24;
    auto always = [&](float* mn, float* mx) { for (int k = 0; k < 3; ++k) { mn[k] = -BIG; mx[k] = BIG; } };
    auto none = [&](float* mn, float* mx, uint32_t& d0, uint32_t& d1) { for (int k = 0; k < 3; ++k) { mn[k] = 0.f; mx[k] = 0.f; } wide_desc(true, 0u, 0u, never, d0, d1); };
    auto inst_child = [&](uint32_t k, float* mn, float* mx, uint32_t& d0, uint32_t& d1) {
        for (int c = 0; c < 3; ++c) { mn[c] = dI[k].rootMin[c]; mx[c] = dI[k].rootMax[c]; }
        d0 = dI[k].rootDesc0; d1 = dI[k].rootDesc1;
        blasAt[binst[k].instanceOffset].owner = k;          // the candidate's instance comes from the triangle
    };
    // fan-out over instances [a, b): returns the child entry for that range
    std::function<uint32_t(uint32_t, uint32_t, float*, float*, uint32_t&, uint32_t&)> range_child =
        [&](uint32_t a, uint32_t b, float* mn, float* mx, uint32_t& d0, uint32_t& d1) -> uint32_t {
            if (b - a == 1) { inst_child(a, mn, mx, d0, d1); return (dI[a].rootDesc1 & WIDE_LEAF) ? 0u : 1u + blasAt[binst[a].instanceOffset].anyNeed; }
            const uint32_t mid = a + (b - a) / 2;
            const uint32_t idx = wideOffset + (uint32_t)dW.size();
            dW.emplace_back();
            DWide w{};
            const uint32_t hl = range_child(a, mid, w.lmin, w.lmax, w.ld0, w.ld1);
            const uint32_t hr = range_child(mid, b, w.rmin, w.rmax, w.rd0, w.rd1);
            dW[idx - wideOffset] = w;
            always(mn, mx);
            wide_desc(false, idx, 0u, never, d0, d1);
            return 1u + std::max(hl, hr);
        };
    // top-level nodes, children first (DFS pre-order: children have larger indices)
    std::vector<uint32_t> uIdx(nTop, 0), uH(nTop, 0);
    for (uint32_t i = nTop; i-- > 0;) {
        const BlobNode& n = tnodes[i];
        if (n.w0 & LEAF_BIT) continue;
        const uint32_t idx = wideOffset + (uint32_t)dW.size();
        dW.emplace_back();
        DWide w{};
        uint32_t h[2] = {0, 0};
        for (int c = 0; c < 2; ++c) {
            const uint32_t ch = c ? n.w1 : n.w0;
            float* mn = c ? w.rmin : w.lmin; float* mx = c ? w.rmax : w.lmax;
            uint32_t& d0 = c ? w.rd0 : w.ld0; uint32_t& d1 = c ? w.rd1 : w.ld1;
            const BlobNode& cn = tnodes[ch];
            if (!(cn.w0 & LEAF_BIT)) {
                for (int k = 0; k < 3; ++k) { mn[k] = cn.bottom[k]; mx[k] = cn.top[k]; }
                wide_desc(false, uIdx[ch], 0u, never, d0, d1);
                h[c] = 1u + uH[ch];
            } else {
                const uint32_t cnt = cn.w2 == TYPE_INST ? (cn.w0 & 0x7fffffffu) : 0u;
                if (cnt == 0) none(mn, mx, d0, d1);
                else {
                    h[c] = range_child(cn.w1, cn.w1 + cnt, mn, mx, d0, d1);      // (one instance: its root test is this child's box test)
                }
            }
        }
        dW[idx - wideOffset] = w;
        uIdx[i] = idx; uH[i] = std::max(h[0], h[1]);
    }
    // super-root: the reference tests the top-level root's own box when it pops it
    DWide sr{};
    for (int k = 0; k < 3; ++k) { sr.lmin[k] = tnodes[0].bottom[k]; sr.lmax[k] = tnodes[0].top[k]; }
    wide_desc(false, uIdx[0], 0u, never, sr.ld0, sr.ld1);
    none(sr.rmin, sr.rmax, sr.rd0, sr.rd1);
    L.s.unifiedRoot = wideOffset + (uint32_t)dW.size();
    dW.push_back(sr);
    L.s.unifiedNeed = uH[0] + 2u;
}

// the owner words the two steps above decided (a fresh derivation: every other triangle keeps the 0xffffffff of import_blas)
void Deriver::write_owners()
{
    for (auto& kv : blasAt) {
        const BlasInfo& bi = kv.second;
        if (bi.owner == 0xffffffffu) continue;
        for (uint32_t t = 0; t < bi.nTris; ++t) L.tris[bi.triBase + t]._p0 = bi.owner;
    }
}

// ---- step 6: quad records ----------------------------------------------------------------------------------------------------
// Quad records (rdx_types.h DQuad): one per wide record, built from the finished wide array -- BLAS nodes and the unified
// tree's records alike.  need[i] = entries the LIFO pool grows by while the subtree of a popped record i is walked alone
// (tight mode of the pool step): the inner entries are pushed together and popped first-entry-first, so
// need = max(k, max_j(entries below j + need[target j])); the halves and the entries inside a half are ordered to
// minimise it (the visiting order is free in the exhaustive walk).
// (not built where the culled walk will run -- large scenes under the automatic rule, or option "cull" 1: the culled walk keeps
// the 64-byte records, and the quad records of a 10 M-triangle scene are 0.6 GB and a second of host time.  Option "cull"
// changed later: the exhaustive walk then uses the 64-byte records until the structure is derived again.)
int Deriver::quad_records()
{
    const std::vector<DWide>& dW = L.wide;
    std::vector<DQuad>& dQ = L.quad;
    const bool wantQuad = want_quad();
    dQ.assign(wantQuad ? dW.size() : 0, DQuad{});
    qneed.assign(dW.size(), 0);
    if (!wantQuad) return 0;
    struct QE { float mn[3], mx[3]; uint32_t d0, d1; };
    auto empty = [](QE& e) { for (int k = 0; k < 3; ++k) { e.mn[k] = 0.f; e.mx[k] = 0.f; } e.d0 = 0u; e.d1 = WIDE_LEAF; };
    auto entry_of = [](const DWide& w, int side, QE& e) {
        for (int k = 0; k < 3; ++k) { e.mn[k] = side ? w.rmin[k] : w.lmin[k]; e.mx[k] = side ? w.rmax[k] : w.lmax[k]; }
        const uint32_t d0 = side ? w.rd0 : w.ld0, d1 = side ? w.rd1 : w.ld1;
        if (d1 & WIDE_LEAF) { e.d0 = wide_slot(d0); e.d1 = WIDE_LEAF | (wide_count(d1) << 24); }
        else { e.d0 = d0; e.d1 = 0u; }
    };
    // the half for child `side` of wide record N
    auto half_of = [&](const DWide& N, int side, QE out[2]) {
        QE c;
        entry_of(N, side, c);
        bool pair = false;
        if (!(c.d1 & WIDE_LEAF) && c.d0 < dW.size()) {
            const DWide& C = dW[c.d0];
            pair = true;
            for (int k = 0; k < 3; ++k)
                if (!(std::min(C.lmin[k], C.rmin[k]) == c.mn[k] && std::max(C.lmax[k], C.rmax[k]) == c.mx[k])) pair = false;
            // an empty entry in C (count-0 leaf with a zero box) would have entered the union above: such a record keeps its own test
            if (pair) {
                entry_of(C, 0, out[0]); entry_of(C, 1, out[1]);
                for (int e = 0; e < 2; ++e) {
                    out[e].d1 |= QUAD_PAIR;
                    if (out[e].d1 & WIDE_LEAF) for (int k = 0; k < 3; ++k) { out[e].mn[k] = c.mn[k]; out[e].mx[k] = c.mx[k]; }
                }
            }
        }
        if (!pair) { out[0] = c; empty(out[1]); }
    };
    // the four entries of a record whose targets are done, in the order of the smallest need -> the record and that need
    auto place = [&](const QE e[4], DQuad& q) -> uint32_t {
        auto nd = [&](const QE& x) -> int { return (x.d1 & WIDE_LEAF) ? -1 : (int)qneed[x.d0]; };
        uint32_t bestNeed = ~0u; int bestArr = 0;
        int ord[4];
        for (int arr = 0; arr < 8; ++arr) {
            quad_order(arr, ord);
            uint32_t inner = 0, need = 0;
            for (int j = 3; j >= 0; --j) {          // j = pop position; `inner` = inner entries popped after j
                const int n = nd(e[ord[j]]);
                if (n < 0) continue;
                need = std::max(need, inner + (uint32_t)n);
                ++inner;
            }
            need = std::max(need, inner);
            if (need < bestNeed) { bestNeed = need; bestArr = arr; }
        }
        quad_order(bestArr, ord);
        for (int hh = 0; hh < 2; ++hh) {
            const QE& a = e[ord[2 * hh]]; const QE& b = e[ord[2 * hh + 1]];
            DWide& w = q.half[hh];
            for (int k = 0; k < 3; ++k) { w.lmin[k] = a.mn[k]; w.lmax[k] = a.mx[k]; w.rmin[k] = b.mn[k]; w.rmax[k] = b.mx[k]; }
            w.ld0 = a.d0; w.ld1 = a.d1; w.rd0 = b.d0; w.rd1 = b.d1;
        }
        return bestNeed;
    };
    // children first: explicit DFS over the records (BLAS records have larger-index children, unified records smaller ones)
    std::vector<uint8_t> state(dW.size(), 0);       // 0 new, 1 open, 2 done
    std::vector<uint32_t> stk;
    for (size_t r = 0; r < dW.size(); ++r) {
        if (state[r]) continue;
        stk.push_back((uint32_t)r);
        while (!stk.empty()) {
            const uint32_t i = stk.back();
            QE e[4];
            half_of(dW[i], 0, e); half_of(dW[i], 1, e + 2);
            if (state[i] == 0) {
                state[i] = 1;
                bool wait = false;
                for (int k = 0; k < 4; ++k)
                    if (!(e[k].d1 & WIDE_LEAF)) {
                        if (e[k].d0 >= dW.size()) return fail("derive_accel: wide record %u refers to record %u of %zu", i, e[k].d0, dW.size());
                        if (state[e[k].d0] == 1) return fail("derive_accel: the wide records are not a tree (cycle through record %u)", e[k].d0);
                        if (state[e[k].d0] == 0) { stk.push_back(e[k].d0); wait = true; }
                    }
                if (wait) continue;
            }
            // all targets done: order the entries and store the record
            qneed[i] = place(e, dQ[i]);
            state[i] = 2;
            stk.pop_back();
        }
    }
    for (auto& kv : blasAt) kv.second.quadNeed = (kv.second.rootDesc1 & WIDE_LEAF) ? 0u : qneed[kv.second.rootDesc0];
    unifiedQuadNeed = L.s.unifiedRoot ? qneed[L.s.unifiedRoot] : 0u;
    // Entry records (step 6b): the half for a "child" that is the BLAS root R itself -- its two children under R's box when
    // that box is their union, else R with its own box -- and an empty second half.  A pool item that points there decides the
    // root test of radiance.cl:61-63 (and, in the pair form, one level below it) by the quad records' own inclusion argument.
    for (auto& kv : blasAt) {
        BlasInfo& bi = kv.second;
        if (bi.rootDesc1 & WIDE_LEAF) continue;
        DWide N{};
        for (int k = 0; k < 3; ++k) { N.lmin[k] = bi.rootMin[k]; N.lmax[k] = bi.rootMax[k]; }
        N.ld0 = bi.rootDesc0; N.ld1 = bi.rootDesc1;
        QE e[4];
        half_of(N, 0, e); empty(e[2]); empty(e[3]);
        bi.entryNeed = place(e, bi.entry);
    }
    return 0;
}

// ---- step 6b: entry records ----------------------------------------------------------------------------------------------------
// One per instance slot, behind the quad records on the device (pool item index = quad records + slot): the entry record of the
// instance's BLAS, or an inert record (four empty entries) for a leaf root -- which the engine never addresses.  They depend on
// the instance's BLAS alone, so an update only re-orders them.
void Deriver::entry_records()
{
    DQuad inert{};
    for (int hh = 0; hh < 2; ++hh) { inert.half[hh].ld1 = WIDE_LEAF; inert.half[hh].rd1 = WIDE_LEAF; }
    L.entries.assign(want_quad() ? nInst : 0u, inert);
    L.entryNeed = 0;
    L.groupFirst = 0;
    for (uint32_t k = std::min(nInst, 256u); k-- > 0;) if (L.groupBits[k >> 5] & (1u << (k & 31u))) L.groupFirst = k;
    for (size_t k = 0; k < L.entries.size(); ++k) {
        const BlasInfo& bi = blasAt[binst[k].instanceOffset];
        if (bi.rootDesc1 & WIDE_LEAF) continue;
        L.entries[k] = bi.entry;
        L.entryNeed = std::max(L.entryNeed, bi.entryNeed);
    }
}

// ---- step 7: top-level needs and the scalars ---------------------------------------------------------------------------------
int Deriver::top_level_needs()
{
    rdx_accel_scalars& s = L.s;
    std::vector<DNode>& dT = L.tnodes;
    uint32_t maxBlasQuad = 0;
    for (auto& kv : blasAt) maxBlasQuad = std::max(maxBlasQuad, kv.second.quadNeed);
    // stack need: TLAS part
    // (cooperative kernel: the instances of a top-level leaf are pushed as 16-bit masks, one entry per 16 instances,
    //  and the entry being consumed is pushed back while one of its instances is walked)
    std::vector<uint32_t> needT(nTop, 0), needC(nTop, 0), needTopOnly(nTop, 0);
    uint32_t maxBlasCoop = 0, maxBlasAny = 0;
    L.ctnodes = dT;
    std::vector<DNode>& dTc = L.ctnodes;
    for (uint32_t i = nTop; i-- > 0;) {
        const BlobNode& n = tnodes[i];
        if (n.w0 & LEAF_BIT) {
            const uint32_t cnt = n.w0 & 0x7fffffffu;
            uint32_t mx = 0, mxc = 0, mxp = 0;
            for (uint32_t k = 0; k < cnt; ++k) {
                const BlasInfo& bi = blasAt[binst[n.w1 + k].instanceOffset];
                mx = std::max(mx, bi.need); mxc = std::max(mxc, bi.coopNeed); maxBlasAny = std::max(maxBlasAny, bi.anyNeed);
                mxp = std::max(mxp, bi.coopNeed + bi.coopPieces);
            }
            maxBlasCoop = std::max(maxBlasCoop, mxc);
            needTopOnly[i] = (cnt + 15u) / 16u;
            needT[i] = (cnt ? cnt - 1 : 0) + mx;
            needC[i] = (cnt + 15u) / 16u + mxp;       // (the cooperative kernel's stack: with the leaf pieces along a path)
        } else {
            needT[i] = std::max(1u + needT[n.w0], needT[n.w1]);   // children have larger indices (DFS pre-order)
            // cooperative kernel: its own copy of the top-level nodes with the smaller-need child in the followed slot
            if (needC[n.w1] < needC[n.w0]) std::swap(dTc[i].w0, dTc[i].w1);
            needC[i] = std::max(1u + needC[dTc[i].w0], needC[dTc[i].w1]);
            needTopOnly[i] = std::max(1u + needTopOnly[dTc[i].w0], needTopOnly[dTc[i].w1]);
        }
    }
    s.stackNeed = std::max(1u, needT[0]) + 1u + maxLeafChunks;
    // oversized leaves are cut into 8-triangle work items: all but the first piece of each child are pushed
    s.coopNeed = std::max(1u, needC[0]) + 1u + 2u * ((std::max(maxLeafTris, 1u) + 7u) / 8u - 1u);
    s.topNeed = std::max(1u, needTopOnly[0]) + 1u;
    // flat top level: <= 64 nodes (one reach bit each); the pending instances of a ray are a bitmap of <= 8 words per lane
    s.topFlat = (nTop <= 64 && nInst <= 256) ? nTop : 0u;
    // spare word of a top-level leaf: it holds instances whose BLAS is a single leaf of <= 8 triangles (pool engine)
    for (uint32_t i = 0; i < nTop; ++i) {
        dT[i].w3 = 0;
        if (!(tnodes[i].w0 & LEAF_BIT)) continue;
        for (uint32_t k = 0; k < (tnodes[i].w0 & 0x7fffffffu); ++k) {
            const DInst& di = L.insts[tnodes[i].w1 + k];
            if ((di.rootDesc1 & WIDE_LEAF) && wide_count(di.rootDesc1) <= 8u) { dT[i].w3 = 1; s.leafRoots = 1; }
        }
    }
    s.nInst = nInst;
    s.topFlatNeed = std::max(1u, (nInst + 31u) / 32u);       // words per lane of the pending-instance bitmap
    s.blasNeed = maxBlasCoop;
    s.blasNeedAny = maxBlasAny;
    for (int k = 0; k < 3; ++k) { s.sceneLo[k] = tnodes[0].bottom[k]; s.sceneHi[k] = tnodes[0].top[k]; }
    s.sbtOffsets = sbtOffsets || hugeLeaf;      // (either way: the reference-order kernel, which reads the blob's own node layout)
    s.quadNeed = maxBlasQuad; s.quadUnifiedNeed = s.unifiedRoot ? unifiedQuadNeed + 1u : 0u;
    s.nWide = total_wide();
    // packed-word limits of the cooperative engines (rdx_types.h); the runtime adds their LDS footprint
    s.coopOK = coopOK && total_tris() <= RDX_COOP_MAX_TRI_SLOTS - 1u && total_wide() < RDX_COOP_MAX_WIDE;
    // per-lane kernels: [need][64 lanes] words of LDS per wave, 64 KB at most
    if (s.stackNeed > 250) return fail("BVH too deep for the LDS traversal stack: %u entries per ray needed, 250 available", s.stackNeed);
    return 0;
}

// ---- the book: what update_accel_layout needs of this derivation ----------------------------------------------------------------
void Deriver::make_book()
{
    AccelBook& B = L.book;
    const auto* th = reinterpret_cast<const BlobTopHeader*>(blob);
    const uint64_t regionStart = (uint64_t)th->instByteOffset + (uint64_t)nInst * sizeof(BlobInst);
    B = AccelBook{};
    B.valid = th->totalBufferSize >= regionStart;
    B.blasRegionBytes = B.valid ? th->totalBufferSize - regionStart : 0;
    B.nInst = nInst; B.nTris = total_tris(); B.nBlasWide = nBlasWide;
    B.maxLeafChunks = maxLeafChunks; B.maxLeafTris = maxLeafTris;
    B.hugeLeaf = hugeLeaf; B.coopBlasOK = coopBlasOK; B.quadBuilt = want_quad();
    for (auto& kv : blasAt) {
        const BlasInfo& bi = kv.second;
        if (kv.first < regionStart) { B.valid = false; break; }
        AccelBlasBlock b{};
        b.relOffset = (uint32_t)(kv.first - regionStart);
        b.nodeBase = bi.nodeBase; b.triBase = bi.triBase; b.nTris = bi.nTris;
        b.need = bi.need; b.coopNeed = bi.coopNeed; b.anyNeed = bi.anyNeed; b.quadNeed = bi.quadNeed; b.coopPieces = bi.coopPieces;
        b.rootDesc0 = bi.rootDesc0; b.rootDesc1 = bi.rootDesc1;
        for (int k = 0; k < 3; ++k) { b.rootMin[k] = bi.rootMin[k]; b.rootMax[k] = bi.rootMax[k]; }
        b.owner = bi.owner;
        b.entry = bi.entry; b.entryNeed = bi.entryNeed;
        B.blocks.push_back(b);
    }
}

} // namespace

int derive_accel_layout(const void* blob, size_t size, const AccelOptions& opt, AccelLayout& out, std::string& err)
{
    out = AccelLayout{};
    Deriver d{static_cast<const uint8_t*>(blob), size, opt, out, err};
    if (d.import_top() || d.instance_records()) return -1;      // (a BLAS is imported when the first instance refers to it)
    d.shared_transform_group();
    d.nBlasWide = (uint32_t)out.wide.size();
    d.unified_tree();
    d.write_owners();
    if (d.quad_records() || d.top_level_needs()) return -1;
    d.entry_records();
    d.make_book();
    return 0;
}

int update_accel_layout(const void* blob, size_t size, const AccelOptions& opt, AccelLayout& inout, AccelUpdate& what, std::string& err)
{
    what = AccelUpdate{};
    const AccelBook& B = inout.book;
    if (!B.valid) return 1;
    AccelLayout N;                  // the top-level part, derived into a layout without BLAS blocks
    Deriver d{static_cast<const uint8_t*>(blob), size, opt, N, err};
    d.update = true; d.wideOffset = d.nBlasWide = B.nBlasWide; d.bookTris = B.nTris;
    if (d.import_top()) return -1;
    const auto* th = reinterpret_cast<const BlobTopHeader*>(blob);
    const uint64_t regionStart = (uint64_t)th->instByteOffset + (uint64_t)d.nInst * sizeof(BlobInst);
    if (d.nInst != B.nInst || th->totalBufferSize < regionStart || th->totalBufferSize - regionStart != B.blasRegionBytes) return 1;
    for (const AccelBlasBlock& b : B.blocks) {
        BlasInfo bi{};
        bi.nodeBase = b.nodeBase; bi.triBase = b.triBase; bi.nTris = b.nTris;
        bi.need = b.need; bi.coopNeed = b.coopNeed; bi.anyNeed = b.anyNeed; bi.quadNeed = b.quadNeed; bi.coopPieces = b.coopPieces;
        bi.rootDesc0 = b.rootDesc0; bi.rootDesc1 = b.rootDesc1;
        for (int k = 0; k < 3; ++k) { bi.rootMin[k] = b.rootMin[k]; bi.rootMax[k] = b.rootMax[k]; }
        bi.users = 0; bi.owner = 0xffffffffu;
        bi.entry = b.entry; bi.entryNeed = b.entryNeed;
        d.blasAt.emplace((uint32_t)(regionStart + b.relOffset), bi);
    }
    d.maxLeafChunks = B.maxLeafChunks; d.maxLeafTris = B.maxLeafTris; d.hugeLeaf = B.hugeLeaf;
    d.coopBlasOK = B.coopBlasOK; d.coopOK = d.coopOK && B.coopBlasOK;
    if (d.instance_records()) return d.needFull ? 1 : -1;
    for (auto& kv : d.blasAt) if (kv.second.users == 0) return 1;
    d.shared_transform_group();
    d.unified_tree();
    // quad records exist for every wide record or for none: a change of that is a change of the BLAS blocks' part too
    if (d.want_quad() != B.quadBuilt) return 1;
    if ((N.s.unifiedRoot != 0) != (inout.s.unifiedRoot != 0)) return 1;
    if (d.top_level_needs()) return -1;
    d.entry_records();

    // what changed
    auto differs = [](const auto& a, const auto& b) { return a.size() != b.size() || (a.size() && std::memcmp(a.data(), b.data(), a.size() * sizeof(a[0])) != 0); };
    what.tnodes = differs(N.tnodes, inout.tnodes); what.ctnodes = differs(N.ctnodes, inout.ctnodes); what.insts = differs(N.insts, inout.insts);
    what.groupBits = std::memcmp(N.groupBits, inout.groupBits, sizeof N.groupBits) != 0;
    what.entries = differs(N.entries, inout.entries);
    size_t bi = 0;
    for (auto& kv : d.blasAt) {     // (the map's order is the blocks' order: both ascend by byte offset)
        const AccelBlasBlock& old = B.blocks[bi++];
        if (kv.second.owner != old.owner && old.nTris) what.owners.push_back(AccelOwnerRange{old.triBase, old.nTris, kv.second.owner});
    }
    what.wideTailFirst = B.nBlasWide;
    what.wideTail = std::move(N.wide);
    what.wideTailChanged = !what.wideTail.empty() || inout.s.nWide != B.nBlasWide;
    N.wide.clear();
    d.make_book();
    inout.tnodes = std::move(N.tnodes); inout.ctnodes = std::move(N.ctnodes); inout.insts = std::move(N.insts);
    std::memcpy(inout.groupBits, N.groupBits, sizeof N.groupBits);
    inout.entries = std::move(N.entries); inout.entryNeed = N.entryNeed; inout.groupFirst = N.groupFirst;
    inout.s = N.s;
    inout.book = std::move(N.book);
    return 0;
}

void apply_accel_update(AccelLayout& L, const AccelUpdate& what)
{
    for (const AccelOwnerRange& r : what.owners)
        for (uint32_t t = 0; t < r.count; ++t) L.tris[r.first + t]._p0 = r.owner;
    L.wide.resize(what.wideTailFirst);
    L.wide.insert(L.wide.end(), what.wideTail.begin(), what.wideTail.end());
}

} // namespace rdx

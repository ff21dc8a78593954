// rdx_runtime.cpp -- host runtime behind the C ABI (include/rdx.h): device/stream singleton,
// buffers, acceleration-structure upload + derived layout, pipeline binding and the per-frame
// wavefront schedule.  Replaces the OpenCL host runtime of the reference
// (radiance/src/radiance.cpp, radiance/src/clcontext.cpp) for the ray-tracing hot path.
#include "../../include/rdx.h"

#include <hip/hip_runtime.h>

#include <algorithm>
#include <cctype>
#include <cmath>
#include <cstdarg>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <map>
#include <memory>
#include <mutex>
#include <cfloat>
#include <chrono>
#include <string>
#include <atomic>
#include <thread>
#include <vector>

#ifndef RDX_SBT_HEADER
#define RDX_SBT_HEADER "sbt_generated.h"      // tools/genSBT.py output (the table this library's stage kernels were built for)
#endif
#ifndef RDX_QUAD_AUTO_MAX_PATHS
#define RDX_QUAD_AUTO_MAX_PATHS (3u << 20)      // option "quad" -1: chunks of at most this many paths walk the quad records (1/4 of a 1080p x 4 spp frame: 2.1 M)
#endif
#ifndef RDX_STOCK_REDUCED_HASH
#define RDX_STOCK_REDUCED_HASH 0xf95635133b09cb3full         // of samples/shader.cl; tools/stock_shader_hash.py prints it
#endif
#include RDX_SBT_HEADER
#include "accel_layout.h"
#include "area.h"
#include "env.h"
#include "bvh_build.h"
#include "denoise.h"
#include "svgf.h"
#include "temporal.h"
#include "device_math.h"
#include "kernels.h"
#include "light_paths.h"
#include "material_eval.h"
#include "scatter.h"
#include "paths.h"
#include "punctual.h"
#include "raygen.h"
#include "rdx_types.h"
#include "shade.h"
#include "user_shader.h"

using namespace rdx;

#define HIP_IGN(expr) do { (void)(expr); } while (0)

// ------------------------------------------------------------------------------------------------
// handles
// ------------------------------------------------------------------------------------------------
constexpr int RDX_MAX_DEVICES = 16;
// option "sort" -1: scenes with at least this many inner BVH nodes are sorted.  Measured with the r02d engine (1080p x 4 spp; unsorted
// / sorted): 10.4 M triangles 56.9 / 54.3 ms (the sorted hand-out makes the traversal launches 9 % faster, the eight sorts cost
// 1.5 ms), Sponza-class 24.5 / 24.6 (break-even), sample1 13.3 / 15.4 (its rays are coherent as they come; the sort scrambles the
// pixel order).
constexpr uint32_t RDX_SORT_AUTO_MIN_WIDE = 1u << 20;      // option "sort" -1: scenes with at least this many inner BVH nodes sort their rays per bounce ...
constexpr uint32_t RDX_SORT_AUTO_MIN_WIDE_FULL = 1u << 15; // ... and so do scenes from this size on for chunks of more than sortMinPaths paths (the sort is two more dependent
                                                           // launches per bounce, four when this was measured: small shards lose with it, and so does a scene that sits in L2 anyway)
struct AccelCache {                // derived traversal layout of one TLAS buffer on one device (accel_layout.h)
    uint64_t version = ~0ull;
    DNode* tnodes = nullptr; DNode* ctnodes = nullptr; DInst* insts = nullptr; DNode* bnodes = nullptr; DTri* tris = nullptr;
    DWide* wide = nullptr;
    DQuad* quad = nullptr;             // null: the quad records were not built
    uint32_t nQuad = 0;                // quad records in `quad`; with `entriesUp` the entry records of the instance slots follow them
    bool entriesUp = false;            // (AccelLayout::entries: a pool item addresses the one of slot i as nQuad + i)
    uint32_t* groupBits = nullptr;     // 9 words
    uint32_t* slotOf = nullptr;        // rdx_resolve_hits: slotOf[instanceIndex] = slot in `insts`, 0xffffffff = no such instance (nInst words)
    rdx_accel_scalars s{};             // coopOK: ... and the engines' LDS footprint fits (derive_accel)
    // rdx_tlas_update: the host side of the layout without its four large arrays (small arrays, scalars, per-BLAS book), the
    // elements tnodes / ctnodes and wide were allocated for, and the device table of the owner-fill kernel
    AccelLayout host;
    size_t topCap = 0, wideCap = 0;
    uint4* ownerTable = nullptr; size_t ownerCap = 0;
    void release()
    {
        for (void* p : {(void*)tnodes, (void*)ctnodes, (void*)insts, (void*)bnodes, (void*)tris, (void*)wide, (void*)quad, (void*)groupBits, (void*)ownerTable, (void*)slotOf})
            if (p) HIP_IGN(hipFree(p));
        tnodes = nullptr; ctnodes = nullptr; insts = nullptr; bnodes = nullptr; tris = nullptr; wide = nullptr; quad = nullptr; groupBits = nullptr;
        ownerTable = nullptr; ownerCap = 0; slotOf = nullptr;
    }
};

struct rdx_buffer_s {
    void* dptr = nullptr;
    size_t size = 0;
    bool owned = true;
    uint64_t version = 0;                  // bumped by every write
    std::vector<uint8_t> shadow;           // host copy of a TLAS blob (valid iff shadowVersion == version)
    uint64_t shadowVersion = ~0ull;
    std::unique_ptr<AccelCache> accel;
    std::vector<rdx_blas> tlasBlas;        // rdx_tlas_build: the BLAS handle of every instance, by index (empty: not a TLAS built here)
    // small parameter buffers (RTProp, camera): a host mirror kept current by the write path, so that TraceRays does
    // not read them back from the device every frame.  Valid only for library-owned buffers whose every byte has been
    // written through the API since creation (device code never writes them); wrapped memory is never mirrored.
    std::vector<uint8_t> mirror;
    bool mirrorValid = false;
    uint32_t imgW = 0, imgH = 0, imgLayers = 0;   // != 0: an RGBA8 image array created by rdx_image_array_create
    // single-process multi-device mode (rdx_init_devices): the copy of this buffer on logical device d >= 1 and the traversal
    // layout derived from it there; device 0 uses dptr / accel
    void* rep[RDX_MAX_DEVICES] = {};
    std::unique_ptr<AccelCache> accelRep[RDX_MAX_DEVICES];
};
struct rdx_sampler_s { uint32_t addressing = 0, filter = 0; };
struct rdx_blas_s { std::unique_ptr<Blas> blas; };
struct rdx_shader_s { std::string name; bool hasRaygen = false;
                      UserProgram* program = nullptr; };   // != null: a user's program, compiled at run time -- as its raygen megakernel, or
                                                           // (program->stages) as the shade stage of the wavefront pipeline around its stage functions

namespace {

struct Context {
    bool initialized = false;
    int device = 0;
    hipStream_t stream = nullptr;
    hipEvent_t evA = nullptr, evB = nullptr, evChunk = nullptr;
    std::string err;
    std::vector<std::unique_ptr<rdx_buffer_s>> buffers;
    std::vector<std::unique_ptr<rdx_blas_s>> blases;
    std::vector<std::unique_ptr<rdx_shader_s>> shaders;
    rdx_shader_s* pipeline = nullptr;
    void* slots[14] = {};
    uint32_t nslots = 0;
    // sharding
    uint32_t rank = 0, world = 1, tileW = 64, tileH = 64;
    uint32_t* ownedPixels = nullptr; uint32_t ownedCount = 0, ownedW = 0, ownedH = 0, ownedRank = 0, ownedWorld = 0,
              ownedTileW = 0, ownedTileH = 0;
    // path streams: up to MAX_GROUPS independent sets of paths in flight (sample groups of one chunk);
    // each has its own streams (s0: generate/extend/shade, s1: shadow beside the next extend), live
    // counts and events, so launches of different groups overlap and cover each other's tails
    struct Group {
        PathStreams ps{};
        size_t cap = 0;
        uint32_t* sortBins = nullptr;       // per-bounce ray sort: scratch (ray_sort_tiles_words(): the two total[] copies and the offset table; kernels.h) ...
        uint32_t sortPhase = 0;             // ... which copy of total[] the next sort of this group counts into (it is zero by then)
        uint32_t* permE = nullptr; size_t permCap = 0;
        unsigned short* sortKey = nullptr;  // per-bounce ray sort: keys of the survivors, written by the shade stage
        size_t stageCap = 0;                // user stage mode: paths the extra streams (shD, shHit, payC ...) hold
        uint32_t* dCounts = nullptr;        // [0] = paths generated, [d+1] = hits of bounce d, [64+d] / [128+d] ray counters
        uint32_t* hCounts = nullptr;        // pinned
        hipStream_t s0 = nullptr, s1 = nullptr;
        hipEvent_t evShade[64] = {}, evShadow[64] = {}, evDone = nullptr;
    };
    static constexpr int MAX_GROUPS = 4;
    Group groups[MAX_GROUPS];
    size_t sampleCap = 0;
    float4* sampleColor = nullptr;
    uint32_t* dCounts = nullptr;            // = groups[0].dCounts (test seams)
    void* gatherStage[4] = {};              // multi-device gather: packed tiles (RGBA8, imageScratch) on this device and their landing buffers on device 0
    size_t gatherCap[4] = {};
    uint32_t* hStatus = nullptr;            // pinned, device-mapped: bit 0 = a traversal wave hit its iteration bound
    uint32_t* dStatus = nullptr;            // its device address
    unsigned long long* dVisit = nullptr;   // 8 words
    uint32_t* dSurfaceInvalid = nullptr;    // rdx_resolve_hits: records that failed the bounds rule, one word
    uint32_t* dShadeCounts = nullptr;       // rdx_shade_hits: [0] = surviving rays (the compaction cursor), [1] = records that failed the bounds rule (also rdx_resolve_materials')
    CameraArgs* dRaygenArgs = nullptr;      // rdx_generate_rays: the camera's per-call constants, written by its first kernel
    uint32_t* dAccumInvalid = nullptr;      // rdx_accumulate: samples whose pixel number is outside the frame, one word
    float4* pathHits = nullptr;             // rdx_trace_paths without `hits`: the first segment's records of one chunk (2 float4 per path)
    size_t pathHitsCap = 0;
    char* lightScratch = nullptr;           // rdx_trace_paths_lights: the streams of one chunk (light_paths.h LightPathStreams), one allocation
    size_t lightScratchCap = 0;             // ... its size in bytes
    unsigned long long* hVisit = nullptr;   // pinned
    // everything rdx_set_option / rdx_set_profiling write, except the builder's knobs below: handed to the other devices'
    // contexts as a whole (rdx_trace_rays)
    struct Options {
        int64_t chunkPaths = 16ll << 20;
        bool countVisits = false, profiling = false;
        int groupsOpt = 0;                      // sample groups in flight: 1..4, 0 = two for chunks small enough to be ramp + drain bound
        int fuse = -1;                          // shadow(d) + extend(d+1) in one launch: 1 / -1 on, 0 off
        int pathMode = 0;                       // 0 = staged wavefront (launch per stage per bounce), 1 = whole paths in one launch
        int inlineLeafRoots = 1;                // pool engine: single-leaf BLASes handled in the flat top-level step (option "inline_leaf_roots")
        int cull = -1;                          // pool engine: culled walk (option "cull"): 1 on, 0 off, -1 = on for scenes of >= 1 M inner nodes
        int textures = 0;                       // option "textures": 1 = the stock shader samples the bound image array
        int userLocalSize = 64;                 // option "user_shader_local_size": work-group size of a user program's launch (the reference uses 1)
        int sortRays = -1;                      // option "sort": per-bounce ray sort: 1 on, 0 off, -1 automatic
        int topFlat = 1;                        // pool engine: evaluate small top-level trees all at once (option "top_flat")
        int groupInstances = 1;                 // pool engine: instances with bit-identical inverse matrices share one ray slot (option "group_instances")
        int groupEntryItems = 1;                // ... and enter the pool as entry items, all pending ones in one instance step (option "group_entry_items")
        int userStages = 1;                     // user programs that differ from the stock one only inside stage functions run on the wavefront pipeline (option "user_stages")
        int64_t sortMinPaths = 3ll << 19;       // chunks of more paths than this (1.5 M) sort the rays of mid-size scenes and use the 7-wave quad kernels (option
                                                // "sort_min_paths"; 4.7 M / 3 M / 1.5 M: 1/2 frame 13.6 / 12.4 / 12.4 ms, 1/4 frame 7.57 / 7.57 / 7.35 ms, Sponza-class)
        int64_t smallChunkPaths = 9ll << 19;    // chunks of at most this many paths (4.7 M) do not fill the chip: two sample groups, 6-wave quad kernels, no ray sort
                                                // (option "small_chunk_paths")
        int quad = 1;                           // pool engine, exhaustive walk: quad records -- two tree levels per fetch (option "quad"): 1 on (default), 0 off,
                                                // -1 = only for chunks the chip is not filled by (<= RDX_QUAD_AUTO_MAX_PATHS paths)
        int unifiedTree = 1;                    // pool engine: large top levels of identity instances are walked by the pool (option "unified_tree")
        int kernel = 3;                         // traversal kernel: 3 cooperative + shared node pool, 2 cooperative, 1 per-lane wide, 0 reference order
        int overlap = 0;                        // extend(d+1) || shadow(d) on two streams (experimental): 1 on, 0 off
    } opt;
    int gpuBuild = 1;                       // BVH builder: large nodes are binned on the GPU (option "gpu_build"); read on g0 only
    int64_t gpuBuildMin = 32768;            // ... nodes (and meshes) of at least this many primitives (option "gpu_build_min")
    std::vector<std::unique_ptr<rdx_sampler_s>> samplers;
    // user programs: the views their image2d_array_t / sampler_t parameters point to (texture.h TexImageView at 0, TexSamplerView
    // at 32), made from slots 11 / 12 and rewritten when what they describe changes (user_tex_views)
    void* texViews = nullptr;
    uint8_t texViewsHost[48] = {};
    bool texViewsValid = false;
    std::string shaderInclude;              // -I for user shader programs (rdx_shader_include_path; the reference's SHADER_LIB_PATH)
    rdx_trace_stats stats{};
    rdx_tlas_update_stats updStats{};       // of the last rdx_tlas_update (g0 only)
    float camAngles[3] = {0, 0, 0}, camTrig[6] = {1, 0, 1, 0, 1, 0};      // camera_args: cos / sin of the camera angles, evaluated on the device
    bool camCached = false;
    uint32_t visitDepth = 0;                // bounces covered by hVisit after a count_visits frame
    uint64_t bounceCounts[65] = {};         // [d] = closest-hit rays of bounce d, [d+1] = hits = shadow rays of bounce d (last frame)
};
// The process has one Context per LOGICAL device.  g0 is device 0 and also the registry (buffers, shaders, descriptor slots,
// options).  Every function below reads `g`, which is the context of the calling thread: g0 on the caller's thread; inside
// rdx_trace_rays in multi-device mode each worker thread points it at its own device's context (streams, path buffers, counters,
// shard) after copying the registry-side fields it needs (slots, pipeline, options).
Context g0;
Context* g_dev[RDX_MAX_DEVICES] = {&g0};     // logical device -> context (entries >= 1 are heap-allocated by rdx_init_devices)
int g_phys[RDX_MAX_DEVICES] = {0};           // logical device -> HIP device ordinal
int g_ndev = 1;
thread_local Context* tl_ctx = &g0;
thread_local int tl_dev = 0;                 // logical device of the calling thread
#define g (*tl_ctx)

inline void* dp(const rdx_buffer_s* b) { return tl_dev == 0 ? b->dptr : b->rep[tl_dev]; }
inline std::unique_ptr<AccelCache>& acc(rdx_buffer_s* b) { return tl_dev == 0 ? b->accel : b->accelRep[tl_dev]; }
inline const std::unique_ptr<AccelCache>& acc(const rdx_buffer_s* b) { return tl_dev == 0 ? b->accel : b->accelRep[tl_dev]; }

int fail(const char* fmt, ...)
{
    // sized to the message (a compiler log of a user shader program runs to thousands of characters)
    va_list ap, ap2; va_start(ap, fmt); va_copy(ap2, ap);
    const int n = vsnprintf(nullptr, 0, fmt, ap); va_end(ap);
    std::string buf((size_t)(n > 0 ? n : 0) + 1, '\0');
    vsnprintf(&buf[0], buf.size(), fmt, ap2); va_end(ap2);
    buf.resize((size_t)(n > 0 ? n : 0));
    g.err = std::move(buf);
    return -1;
}
int fail_str(const std::string& text) { g.err = text; return -1; }
#define HIP_OK(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) return fail("HIP error: '%s' returned %d (%s)", #expr, (int)_e, hipGetErrorString(_e)); } while (0)
#define HIP_OKP(expr) do { hipError_t _e = (expr); if (_e != hipSuccess) { fail("HIP error: '%s' returned %d (%s)", #expr, (int)_e, hipGetErrorString(_e)); return nullptr; } } while (0)

bool known_buffer(const void* h)
{
    for (auto& b : g0.buffers) if (b.get() == h) return true;
    return false;
}

// ---- derived traversal layout ------------------------------------------------------------------
// beyond the packed-word limits of the cooperative engines or their LDS footprint the per-lane wide kernel runs
bool runtime_coop_ok(const rdx_accel_scalars& S)
{
    return S.coopOK && coop_lds_words(S.coopNeed) <= RDX_LDS_WORDS_PER_WAVE_MAX &&
           pool_lds_words(std::max(S.topNeed, S.topFlatNeed), std::max({S.blasNeed, S.blasNeedAny, S.quadNeed, S.quadUnifiedNeed})) <= RDX_LDS_WORDS_PER_WAVE_MAX;
}

// HitData.instanceIndex is the instance's number in the caller's array (BlobInst.instanceID); the layout's instance records are
// ordered by slot, the order of the top-level leaves.  rdx_resolve_hits finds the record through this table.  An index no instance
// carries (blobs this library did not build may hold anything) maps to 0xffffffff; of two instances with one index the first slot.
std::vector<uint32_t> slot_table(const std::vector<DInst>& insts)
{
    std::vector<uint32_t> t(insts.size(), 0xffffffffu);
    for (size_t k = insts.size(); k-- > 0;)
        if (insts[k].instanceID < t.size()) t[insts[k].instanceID] = (uint32_t)k;
    return t;
}

// accel_layout.cpp derives it on the host; here it is uploaded to the calling thread's device
int derive_accel(rdx_buffer_s* tb)
{
    if (acc(tb) && acc(tb)->version == tb->version) return 0;
    // host copy of the blob
    if (tb->shadowVersion != tb->version) {
        tb->shadow.resize(tb->size);
        HIP_OK(hipMemcpy(tb->shadow.data(), tb->dptr, tb->size, hipMemcpyDeviceToHost));
        tb->shadowVersion = tb->version;
    }
    AccelLayout L;
    std::string err;
    if (derive_accel_layout(tb->shadow.data(), tb->shadow.size(), AccelOptions{g.opt.quad, g.opt.cull}, L, err)) return fail_str(err);
    auto ac = std::make_unique<AccelCache>();
    ac->s = L.s;
    auto up = [&](auto*& dptr, const auto* src, size_t n, size_t cap = 0) -> hipError_t {
        const size_t elem = sizeof(*src);
        hipError_t e = hipMalloc(reinterpret_cast<void**>(&dptr), std::max<size_t>({n, cap, 1}) * elem);
        if (e != hipSuccess) return e;
        return n ? hipMemcpy(dptr, src, n * elem, hipMemcpyHostToDevice) : hipSuccess;
    };
    // (a binary tree over nInst instances has at most 2 nInst - 1 nodes: room for every top level rdx_tlas_update can bring)
    ac->topCap = std::max<size_t>(L.tnodes.size(), 2 * (size_t)L.s.nInst);
    ac->wideCap = L.wide.size();
    HIP_OK(up(ac->tnodes, L.tnodes.data(), L.tnodes.size(), ac->topCap));
    HIP_OK(up(ac->ctnodes, L.ctnodes.data(), L.ctnodes.size(), ac->topCap));
    HIP_OK(up(ac->insts, L.insts.data(), L.insts.size()));
    HIP_OK(up(ac->bnodes, L.bnodes.data(), L.bnodes.size()));
    HIP_OK(up(ac->tris, L.tris.data(), L.tris.size()));
    HIP_OK(up(ac->wide, L.wide.data(), L.wide.size()));
    if (!L.quad.empty()) {
        // the entry records sit behind the quad records, where a pool item's index reaches them -- unless that index would not fit
        ac->nQuad = (uint32_t)L.quad.size();
        ac->entriesUp = !L.entries.empty() && L.quad.size() + L.entries.size() < RDX_COOP_MAX_WIDE;
        HIP_OK(up(ac->quad, L.quad.data(), L.quad.size(), L.quad.size() + (ac->entriesUp ? L.entries.size() : 0)));
        if (ac->entriesUp) HIP_OK(hipMemcpy(ac->quad + ac->nQuad, L.entries.data(), L.entries.size() * sizeof(DQuad), hipMemcpyHostToDevice));
    }
    HIP_OK(up(ac->groupBits, L.groupBits, 9));
    const std::vector<uint32_t> slots = slot_table(L.insts);
    HIP_OK(up(ac->slotOf, slots.data(), slots.size()));
    const rdx_accel_scalars& S = ac->s;
    ac->s.coopOK = runtime_coop_ok(S);
    if (std::getenv("RDX_VERBOSE"))
        std::fprintf(stderr, "[rdx] accel: %zu top nodes, %u instances, %zu wide nodes, %zu triangle slots, stack need %u (cooperative kernel %u = top %u + BLAS %u; quad walk %u)\n",
                     L.tnodes.size(), S.nInst, L.wide.size(), L.tris.size(), S.stackNeed, S.coopNeed, S.topNeed, S.blasNeed, S.quadNeed);
    ac->version = tb->version;
    // kept for rdx_tlas_update: everything but the four large arrays
    std::vector<DNode>().swap(L.bnodes); std::vector<DTri>().swap(L.tris); std::vector<DWide>().swap(L.wide); std::vector<DQuad>().swap(L.quad);
    ac->host = std::move(L);
    if (acc(tb)) acc(tb)->release();
    acc(tb) = std::move(ac);
    return 0;
}

// smallChunk: the caller's launches will not fill the chip (trace_rays_device: chunks of <= RDX_QUAD_AUTO_MAX_PATHS paths)
AccelView view_of(const rdx_buffer_s* tb, bool smallChunk = false)
{
    AccelView v{};
    v.tnodes = acc(tb)->tnodes; v.ctnodes = acc(tb)->ctnodes; v.insts = acc(tb)->insts; v.bnodes = acc(tb)->bnodes; v.tris = acc(tb)->tris;
    v.wide = acc(tb)->wide;
    v.status = g.dStatus;
    v.kernel = acc(tb)->s.sbtOffsets ? 0u : (g.opt.kernel >= 2 && !acc(tb)->s.coopOK) ? 1u : (uint32_t)g.opt.kernel;
    v.stackNeed = acc(tb)->s.stackNeed;
    v.coopNeed = acc(tb)->s.coopNeed;
    // culled walk (docs/CULLED_WALK.md): with the conditioning gate that makes it exact it pays on the scene whose BVH lives in HBM
    // (10.4 M triangles: 66.2 vs 72.1 ms) and not on scenes that fit the caches (Sponza-class: 25.9 vs 25.3 ms exhaustive -- the
    // gate's ~45 vector instructions per node cost what the skipped triangle tests save) -- hence the size rule
    v.cull = (v.kernel == 3 && (g.opt.cull > 0 || (g.opt.cull < 0 && acc(tb)->s.nWide >= RDX_CULL_AUTO_MIN_WIDE))) ? 1u : 0u;
    v.topNeed = acc(tb)->s.topNeed; v.blasNeed = v.cull ? acc(tb)->s.blasNeedAny : acc(tb)->s.blasNeed;
    v.topFlat = g.opt.topFlat ? acc(tb)->s.topFlat : 0u;
    v.numInsts = acc(tb)->s.nInst;
    if (v.topFlat) v.topNeed = acc(tb)->s.topFlatNeed;          // flat top level: words per lane of the pending-instance bitmap
    v.leafRoots = (v.topFlat && g.opt.inlineLeafRoots && acc(tb)->s.leafRoots) ? 1u : 0u;
    v.unifiedRoot = 0;
    if (v.kernel == 3 && !v.topFlat && g.opt.unifiedTree && acc(tb)->s.unifiedRoot) {
        // unified tree: no top-level state per lane at all (one bitmap word stays allocated: the engine's flat-mode bookkeeping)
        v.unifiedRoot = acc(tb)->s.unifiedRoot;
        v.topFlat = 1u; v.topNeed = 1u; v.leafRoots = 0u;
        v.blasNeed = acc(tb)->s.unifiedNeed;
    }
    // exhaustive walk of the pool engine: quad records, two tree levels per fetch (option "quad"; the culled walk keeps the
    // wide records, whose children carry the normal cones)
    v.quad = nullptr;
    // (not for the unified tree: its always-entered fan-outs gain nothing from a second level per item -- 39.4 vs 35.4 ms on the
    // 400-instance scene)
    v.quadWaves = 6u;
    v.groupCount = (v.topFlat && !v.unifiedRoot && g.opt.groupInstances) ? acc(tb)->s.groupCount : 0u;
    v.groupBits = acc(tb)->groupBits;
    v.entryBase = 0u; v.groupFirst = 0u;
    if (v.kernel == 3 && !v.cull && acc(tb)->quad && !v.unifiedRoot && (g.opt.quad > 0 || (g.opt.quad < 0 && smallChunk))) {
        v.quad = acc(tb)->quad;
        uint32_t need = std::max(acc(tb)->s.quadNeed, v.blasNeed);
        // the group's instances enter the pool as entry items (option "group_entry_items"; traverse_pool.h): the pool is sized
        // for a walk that starts at an entry record, too
        if (g.opt.groupEntryItems && v.groupCount && acc(tb)->entriesUp) {
            v.entryBase = acc(tb)->nQuad;
            v.groupFirst = acc(tb)->host.groupFirst;
            need = std::max(need, acc(tb)->host.entryNeed);
        }
        v.quadWaves = (!smallChunk && pool_lds_words(v.topNeed, need) <= 1462u) ? 7u : 6u;      // (7 waves: 160 KB / 28)
        // (launches without a quad variant walk the wide records on the same view)
        v.blasNeed = need;
    }
    return v;
}

// ---- path streams --------------------------------------------------------------------------------
int ensure_group(Context::Group& G, size_t paths)
{
    if (paths <= G.cap) return 0;
    float4** arr[] = {&G.ps.rayO, &G.ps.rayD, &G.ps.thr, &G.ps.col, &G.ps.hitA, &G.ps.nRayO, &G.ps.nRayD,
                      &G.ps.nThr, &G.ps.nCol, &G.ps.shO, &G.ps.colLit, &G.ps.colSh};
    for (auto a : arr) { if (*a) HIP_IGN(hipFree(*a)); *a = nullptr; }
    if (G.ps.hitInst) HIP_IGN(hipFree(G.ps.hitInst));
    G.ps.hitInst = nullptr;
    G.cap = 0;
    for (auto a : arr) HIP_OK(hipMalloc(reinterpret_cast<void**>(a), paths * sizeof(float4)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&G.ps.hitInst), paths * sizeof(uint32_t)));
    G.cap = paths;
    return 0;
}

int ensure_samples(size_t samplesTimesPixels)
{
    if (samplesTimesPixels <= g.sampleCap) return 0;
    if (g.sampleColor) HIP_IGN(hipFree(g.sampleColor));
    g.sampleColor = nullptr; g.sampleCap = 0;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.sampleColor), samplesTimesPixels * sizeof(float4)));
    g.sampleCap = samplesTimesPixels;
    return 0;
}

// pixels owned by (rank, world) for a w x h image, ascending tile id, row-major inside a tile
void owned_pixel_list(uint32_t w, uint32_t h, uint32_t tileW, uint32_t tileH, uint32_t rank, uint32_t world,
                      std::vector<uint32_t>& out)
{
    const uint32_t tilesX = (w + tileW - 1) / tileW, tilesY = (h + tileH - 1) / tileH;
    out.clear();
    for (uint32_t t = rank; t < tilesX * tilesY; t += world) {
        const uint32_t x0 = (t % tilesX) * tileW, y0 = (t / tilesX) * tileH;
        for (uint32_t y = y0; y < std::min(h, y0 + tileH); ++y)
            for (uint32_t x = x0; x < std::min(w, x0 + tileW); ++x) out.push_back(y * w + x);
    }
}

int ensure_owned(uint32_t w, uint32_t h)
{
    if (g.world <= 1) { g.ownedCount = w * h; return 0; }
    if (g.ownedPixels && g.ownedW == w && g.ownedH == h && g.ownedRank == g.rank && g.ownedWorld == g.world &&
        g.ownedTileW == g.tileW && g.ownedTileH == g.tileH)
        return 0;
    std::vector<uint32_t> px;
    owned_pixel_list(w, h, g.tileW, g.tileH, g.rank, g.world, px);
    if (g.ownedPixels) HIP_IGN(hipFree(g.ownedPixels));
    g.ownedPixels = nullptr;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.ownedPixels), std::max<size_t>(px.size(), 1) * 4));
    if (!px.empty()) HIP_OK(hipMemcpy(g.ownedPixels, px.data(), px.size() * 4, hipMemcpyHostToDevice));
    g.ownedCount = (uint32_t)px.size();
    g.ownedW = w; g.ownedH = h; g.ownedRank = g.rank; g.ownedWorld = g.world; g.ownedTileW = g.tileW; g.ownedTileH = g.tileH;
    return 0;
}

int camera_args(const PhysicalCamera& cam, CameraArgs& C)
{
    C.cam = cam;
    // EulerX/Y/ZToMat4x4 (math.cl:185-252): per-frame constants.  cos / sin are evaluated ON THE DEVICE (k_euler_trig) so
    // that they are the OCML values the reference's own cos() / sin() give on this GPU -- libm's differ in the last bit
    // and every primary ray would with them; the six values are cached until the camera angles change.
    float (&cachedAngles)[3] = g.camAngles; float (&cachedTrig)[6] = g.camTrig; bool& cached = g.camCached;
    if (!cached || std::memcmp(cachedAngles, &cam.wx, 12) != 0) {
        float* d6 = nullptr;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&d6), 6 * sizeof(float)));
        launch_euler_trig(g.stream, cam.wx, cam.wy, cam.wz, d6);
        hipError_t e = hipGetLastError();
        if (e == hipSuccess) e = hipMemcpyAsync(cachedTrig, d6, sizeof cachedTrig, hipMemcpyDeviceToHost, g.stream);
        if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
        HIP_IGN(hipFree(d6));
        HIP_OK(e);
        std::memcpy(cachedAngles, &cam.wx, 12);
        cached = true;
    }
    const float cx = cachedTrig[0], sx = cachedTrig[1], cy = cachedTrig[2], sy = cachedTrig[3], cz = cachedTrig[4], sz = cachedTrig[5];
    const float rx[16] = {1, 0, 0, 0, 0, cx, -sx, 0, 0, sx, cx, 0, 0, 0, 0, 1};
    const float ry[16] = {cy, 0, sy, 0, 0, 1, 0, 0, -sy, 0, cy, 0, 0, 0, 0, 1};
    const float rz[16] = {cz, -sz, 0, 0, sz, cz, 0, 0, 0, 0, 1, 0, 0, 0, 0, 1};
    std::memcpy(C.rotX, rx, 64); std::memcpy(C.rotY, ry, 64); std::memcpy(C.rotZ, rz, 64);
    return 0;
}

// the sampler `h` (slot 12) as TexView::flags bits: addressing mode and filter (no TEX_ENABLED); false if `h` is not a sampler
bool sampler_bits(const void* h, uint32_t& bits)
{
    for (auto& sm : g.samplers)
        if (sm.get() == h) {
            const uint32_t mode = sm->addressing == 0x1131 ? TEX_ADDR_CLAMP_TO_EDGE : sm->addressing == 0x1132 ? TEX_ADDR_CLAMP
                                : sm->addressing == 0x1134 ? TEX_ADDR_MIRRORED : TEX_ADDR_REPEAT;
            bits = (sm->filter == 0x1141 ? TEX_LINEAR : 0u) | (mode << TEX_ADDR_SHIFT);
            return true;
        }
    return false;
}

// device addresses of the image and sampler views a user program's entry point passes for its image2d_array_t / sampler_t
// parameters (csrc/user_texture.hip reads them).  Never null: a NULL slot 11 (or a buffer that is not an image array) is a zero
// image view, a NULL slot 12 (or no sampler) a zero sampler view -- reads return (0, 0, 0, 0), queries 0.  Independent of option
// "textures", which switches the stock shader's reads only.  The block is rewritten, in stream order, when its contents change:
// another descriptor set, image or sampler.
int user_tex_views(void*& image, void*& sampler)
{
    TexImageView iv{nullptr, 0, 0, 0, 0};
    TexSamplerView sv{0, {0, 0, 0}};
    if (g.slots[11] && known_buffer(g.slots[11])) {
        const auto* img = static_cast<const rdx_buffer_s*>(g.slots[11]);
        if (img->imgW && img->imgH && img->imgLayers) iv = TexImageView{static_cast<const uint8_t*>(dp(img)), img->imgW, img->imgH, img->imgLayers, 0};
    }
    uint32_t bits = 0;
    if (g.slots[12] && sampler_bits(g.slots[12], bits)) sv.flags = TEX_ENABLED | bits;
    uint8_t host[48] = {};
    static_assert(sizeof(TexImageView) <= 32 && sizeof(TexSamplerView) <= 16, "view block layout");
    std::memcpy(host, &iv, sizeof iv);
    std::memcpy(host + 32, &sv, sizeof sv);
    if (!g.texViews) { HIP_OK(hipMalloc(&g.texViews, sizeof host)); g.texViewsValid = false; }
    if (!g.texViewsValid || std::memcmp(host, g.texViewsHost, sizeof host)) {
        std::memcpy(g.texViewsHost, host, sizeof host);
        HIP_OK(hipMemcpyAsync(g.texViews, g.texViewsHost, sizeof host, hipMemcpyHostToDevice, g.stream));
        HIP_OK(hipStreamSynchronize(g.stream));          // (the host copy may change again before a later call)
        g.texViewsValid = true;
    }
    image = g.texViews;
    sampler = static_cast<uint8_t*>(g.texViews) + 32;
    return 0;
}

int scene_args(SceneArgs& sc)
{
    for (int i : {4, 5, 7, 8, 9, 10})
        if (!g.slots[i] || !known_buffer(g.slots[i])) return fail("descriptor slot %d is not a buffer", i);
    auto ptr = [&](int i) { return dp(static_cast<rdx_buffer_s*>(g.slots[i])); };
    sc.scene = static_cast<const SceneProperties*>(ptr(4));
    sc.meshInfo = static_cast<const MeshInfo*>(ptr(5));
    sc.indexData = static_cast<const uint32_t*>(ptr(7));
    sc.uvData = static_cast<const float*>(ptr(8));
    sc.normalData = static_cast<const float*>(ptr(9));
    sc.materials = static_cast<const Material*>(ptr(10));
    if (static_cast<rdx_buffer_s*>(g.slots[4])->size < sizeof(SceneProperties)) return fail("scene buffer smaller than SceneProperties");
    // slots 11 / 12: texture array + sampler.  Read only when option "textures" is on (the live reference shader has its
    // reads stubbed to 0, samples/shader.cl:379-445)
    sc.tex = TexView{nullptr, 0, 0, 0, 0};
    if (g.opt.textures && g.slots[11] && known_buffer(g.slots[11])) {
        const auto* img = static_cast<const rdx_buffer_s*>(g.slots[11]);
        if (img->imgW && img->imgH && img->imgLayers) {
            uint32_t bits = TEX_ADDR_REPEAT << TEX_ADDR_SHIFT;     // no sampler bound: repeat + nearest
            (void)sampler_bits(g.slots[12], bits);
            sc.tex = TexView{static_cast<const uint8_t*>(dp(img)), img->imgW, img->imgH, img->imgLayers, TEX_ENABLED | bits};
        }
    }
    return 0;
}

// The status word the traversal kernels raise (bit 0: a wave hit its iteration bound) is tested and cleared after EVERY
// synchronise that follows a traversal launch -- frames and the batch seams alike -- so that a raised bit is reported to
// the call that caused it and never to the next one.
bool take_status()
{
    if (!g.hStatus || !*static_cast<volatile uint32_t*>(g.hStatus)) return false;
    *g.hStatus = 0;
    return true;
}

struct StageTimer {
    // per-stage HIP-event timing (profiling mode): events are recorded around each launch and
    // resolved after the frame so that the stream is never drained in the middle
    struct Span { hipEvent_t a, b; float* dst; };
    std::vector<Span> spans;
    std::vector<hipEvent_t> pool;
    size_t used = 0;
    hipEvent_t get()
    {
        if (used == pool.size()) { hipEvent_t e; HIP_IGN(hipEventCreate(&e)); pool.push_back(e); }
        return pool[used++];
    }
    void begin(float* dst, hipStream_t st = nullptr) { if (!g.opt.profiling) return; Span s{get(), get(), dst}; HIP_IGN(hipEventRecord(s.a, st ? st : g.stream)); spans.push_back(s); }
    void end(hipStream_t st = nullptr) { if (!g.opt.profiling) return; HIP_IGN(hipEventRecord(spans.back().b, st ? st : g.stream)); }
    void resolve()
    {
        for (auto& s : spans) { float ms = 0; HIP_IGN(hipEventElapsedTime(&ms, s.a, s.b)); *s.dst += ms; }
        spans.clear(); used = 0;
    }
    ~StageTimer() { for (hipEvent_t e : pool) HIP_IGN(hipEventDestroy(e)); }      // (worker threads of the multi-device mode end per frame)
};
thread_local StageTimer g_timer;

} // namespace

// ------------------------------------------------------------------------------------------------
// platform
// ------------------------------------------------------------------------------------------------
// streams, events, counters of the calling thread's context `g` on HIP device `device` (which must be current)
static int init_device_state(int device)
{
    g.device = device;
    HIP_OK(hipStreamCreateWithFlags(&g.stream, hipStreamNonBlocking));
    HIP_OK(hipEventCreate(&g.evA));
    HIP_OK(hipEventCreate(&g.evB));
    HIP_OK(hipEventCreateWithFlags(&g.evChunk, hipEventDisableTiming));
    for (int k = 0; k < Context::MAX_GROUPS; ++k) {
        Context::Group& G = g.groups[k];
        if (k == 0) G.s0 = g.stream; else HIP_OK(hipStreamCreateWithFlags(&G.s0, hipStreamNonBlocking));
        HIP_OK(hipStreamCreateWithFlags(&G.s1, hipStreamNonBlocking));
        for (int i = 0; i < 64; ++i) {
            HIP_OK(hipEventCreateWithFlags(&G.evShade[i], hipEventDisableTiming));
            HIP_OK(hipEventCreateWithFlags(&G.evShadow[i], hipEventDisableTiming));
        }
        HIP_OK(hipEventCreateWithFlags(&G.evDone, hipEventDisableTiming));
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&G.dCounts), 256 * sizeof(uint32_t)));
        HIP_OK(hipMemset(G.dCounts, 0, 256 * sizeof(uint32_t)));
        HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&G.hCounts), 256 * sizeof(uint32_t), hipHostMallocDefault));
    }
    g.dCounts = g.groups[0].dCounts;
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&g.hStatus), 64, hipHostMallocMapped));
    *g.hStatus = 0;
    HIP_OK(hipHostGetDevicePointer(reinterpret_cast<void**>(&g.dStatus), g.hStatus, 0));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.dVisit), 64 * 8 * sizeof(unsigned long long)));     // [bounce][class*4 + kind]
    HIP_OK(hipHostMalloc(reinterpret_cast<void**>(&g.hVisit), 64 * 8 * sizeof(unsigned long long), hipHostMallocDefault));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.dSurfaceInvalid), sizeof(uint32_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.dShadeCounts), 2 * sizeof(uint32_t)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.dRaygenArgs), sizeof(CameraArgs)));
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.dAccumInvalid), sizeof(uint32_t)));
    g.initialized = true;
    return 0;
}

static void release_device_state()
{
    if (!g.initialized) return;
    HIP_IGN(hipSetDevice(g.device));
    HIP_IGN(hipStreamSynchronize(g.stream));
    for (int k = 0; k < Context::MAX_GROUPS; ++k) {
        Context::Group& G = g.groups[k];
        float4** arr[] = {&G.ps.rayO, &G.ps.rayD, &G.ps.thr, &G.ps.col, &G.ps.hitA, &G.ps.nRayO, &G.ps.nRayD, &G.ps.nThr,
                          &G.ps.nCol, &G.ps.shO, &G.ps.colLit, &G.ps.colSh};
        for (auto a : arr) { if (*a) HIP_IGN(hipFree(*a)); *a = nullptr; }
        if (G.ps.hitInst) HIP_IGN(hipFree(G.ps.hitInst));
        if (G.dCounts) HIP_IGN(hipFree(G.dCounts));
        if (G.hCounts) HIP_IGN(hipHostFree(G.hCounts));
        if (G.sortBins) HIP_IGN(hipFree(G.sortBins));
        if (G.permE) HIP_IGN(hipFree(G.permE));
        if (G.sortKey) HIP_IGN(hipFree(G.sortKey));
        G.sortKey = nullptr;
        for (int i = 0; i < 64; ++i) { HIP_IGN(hipEventDestroy(G.evShade[i])); HIP_IGN(hipEventDestroy(G.evShadow[i])); }
        HIP_IGN(hipEventDestroy(G.evDone));
        HIP_IGN(hipStreamSynchronize(G.s1)); HIP_IGN(hipStreamDestroy(G.s1));
        if (k > 0) { HIP_IGN(hipStreamSynchronize(G.s0)); HIP_IGN(hipStreamDestroy(G.s0)); }
    }
    if (g.sampleColor) HIP_IGN(hipFree(g.sampleColor));
    if (g.ownedPixels) HIP_IGN(hipFree(g.ownedPixels));
    if (g.texViews) HIP_IGN(hipFree(g.texViews));
    g.texViews = nullptr; g.texViewsValid = false;
    for (void* p : g.gatherStage) if (p) HIP_IGN(hipFree(p));
    if (g.hStatus) HIP_IGN(hipHostFree(g.hStatus));
    g.hStatus = nullptr; g.dStatus = nullptr;
    if (g.dVisit) HIP_IGN(hipFree(g.dVisit));
    if (g.hVisit) HIP_IGN(hipHostFree(g.hVisit));
    if (g.dSurfaceInvalid) HIP_IGN(hipFree(g.dSurfaceInvalid));
    g.dSurfaceInvalid = nullptr;
    if (g.dShadeCounts) HIP_IGN(hipFree(g.dShadeCounts));
    g.dShadeCounts = nullptr;
    if (g.dRaygenArgs) HIP_IGN(hipFree(g.dRaygenArgs));
    g.dRaygenArgs = nullptr;
    if (g.dAccumInvalid) HIP_IGN(hipFree(g.dAccumInvalid));
    g.dAccumInvalid = nullptr;
    if (g.pathHits) HIP_IGN(hipFree(g.pathHits));
    g.pathHits = nullptr; g.pathHitsCap = 0;
    if (g.lightScratch) HIP_IGN(hipFree(g.lightScratch));
    g.lightScratch = nullptr; g.lightScratchCap = 0;
    HIP_IGN(hipEventDestroy(g.evA)); HIP_IGN(hipEventDestroy(g.evB)); HIP_IGN(hipEventDestroy(g.evChunk));
    HIP_IGN(hipStreamDestroy(g.stream));
}

// GPU-assisted candidate evaluation of the BVH builder (bvh_build.h GpuBinner; reference: the candidate loop of
// radiance/src/bvh.cpp:90-205): the primitives of a large mesh live on the device while it is built, the binning pass of its
// large nodes is one kernel (kernels.hip k_bvh_bin).  Builder threads share one set of staging buffers behind a mutex; a call
// is a few hundred microseconds.
struct HipBinner final : GpuBinner {
    std::mutex m;
    std::map<uint64_t, float*> sets;
    uint64_t next = 1;
    std::atomic<uint64_t> calls{0};     // nodes binned on the device (rdx_debug_gpu_bin_calls)
    int device = 0;
    uint32_t* dWork = nullptr; size_t workCap = 0;
    float* dCand = nullptr; uint32_t* dOut = nullptr; uint32_t* hOut = nullptr;
    hipStream_t st = nullptr;
    static constexpr size_t kSlots = 1025, kOutWords = 3 * 7 * kSlots;
    bool ready()
    {
        if (st) return true;
        if (hipStreamCreateWithFlags(&st, hipStreamNonBlocking) != hipSuccess) { st = nullptr; return false; }
        if (hipMalloc(reinterpret_cast<void**>(&dCand), 3 * 1024 * sizeof(float)) != hipSuccess ||
            hipMalloc(reinterpret_cast<void**>(&dOut), kOutWords * 4) != hipSuccess ||
            hipHostMalloc(reinterpret_cast<void**>(&hOut), kOutWords * 4, hipHostMallocDefault) != hipSuccess) { shutdown(); return false; }
        return true;
    }
    void shutdown()
    {
        std::lock_guard<std::mutex> lk(m);
        for (auto& kv : sets) HIP_IGN(hipFree(kv.second));
        sets.clear();
        if (dWork) HIP_IGN(hipFree(dWork));
        if (dCand) HIP_IGN(hipFree(dCand));
        if (dOut) HIP_IGN(hipFree(dOut));
        if (hOut) HIP_IGN(hipHostFree(hOut));
        if (st) HIP_IGN(hipStreamDestroy(st));
        dWork = nullptr; workCap = 0; dCand = nullptr; dOut = nullptr; hOut = nullptr; st = nullptr;
    }
    uint64_t upload(const float* prims9, uint32_t n) override
    {
        std::lock_guard<std::mutex> lk(m);
        if (hipSetDevice(device) != hipSuccess || !ready()) return 0;
        float* d = nullptr;
        if (hipMalloc(reinterpret_cast<void**>(&d), (size_t)n * 36) != hipSuccess) return 0;
        if (hipMemcpy(d, prims9, (size_t)n * 36, hipMemcpyHostToDevice) != hipSuccess) { HIP_IGN(hipFree(d)); return 0; }
        sets[next] = d;
        return next++;
    }
    void release(uint64_t h) override
    {
        std::lock_guard<std::mutex> lk(m);
        auto it = sets.find(h);
        if (it == sets.end()) return;
        HIP_IGN(hipSetDevice(device));
        HIP_IGN(hipFree(it->second));
        sets.erase(it);
    }
    bool bin(uint64_t h, const uint32_t* work, size_t n, const std::vector<float> cand[3], std::vector<float>& out) override
    {
        std::lock_guard<std::mutex> lk(m);
        auto it = sets.find(h);
        if (it == sets.end() || n == 0 || n > 0xffffffffull) return false;
        if (hipSetDevice(device) != hipSuccess || !ready()) return false;
        uint32_t K[3];
        for (int a = 0; a < 3; ++a) { K[a] = (uint32_t)cand[a].size(); if (K[a] > 1024u) return false; }
        if (workCap < n) {
            if (dWork) HIP_IGN(hipFree(dWork));
            dWork = nullptr; workCap = 0;
            if (hipMalloc(reinterpret_cast<void**>(&dWork), n * 4) != hipSuccess) return false;
            workCap = n;
        }
        bool ok = hipMemcpyAsync(dWork, work, n * 4, hipMemcpyHostToDevice, st) == hipSuccess;
        for (int a = 0; a < 3 && ok; ++a)
            if (K[a]) ok = hipMemcpyAsync(dCand + 1024 * a, cand[a].data(), K[a] * sizeof(float), hipMemcpyHostToDevice, st) == hipSuccess;
        if (!ok) { HIP_IGN(hipStreamSynchronize(st)); return false; }
        launch_bvh_bin(st, it->second, dWork, (uint32_t)n, dCand, K, dOut);
        ok = hipMemcpyAsync(hOut, dOut, kOutWords * 4, hipMemcpyDeviceToHost, st) == hipSuccess;
        if (hipStreamSynchronize(st) != hipSuccess || !ok || hipGetLastError() != hipSuccess) return false;
        calls.fetch_add(1);
        out.clear();
        for (int a = 0; a < 3; ++a) {
            if (!K[a]) continue;
            const uint32_t* o = hOut + (size_t)a * 7 * kSlots;
            const size_t base = out.size(), nb = K[a] + 1u;
            out.resize(base + 7 * nb);
            for (size_t b = 0; b < nb; ++b) {
                std::memcpy(&out[base + b], &o[b], 4);
                float* q = &out[base + nb + 6 * b];
                for (int k = 0; k < 6; ++k) {
                    if (o[b] == 0u) { q[k] = k < 3 ? FLT_MAX : -FLT_MAX; continue; }
                    const uint32_t key = o[(size_t)(1 + k) * kSlots + b];
                    const uint32_t bits = (key & 0x80000000u) ? (key ^ 0x80000000u) : ~key;
                    std::memcpy(&q[k], &bits, 4);
                }
            }
        }
        return true;
    }
};
static HipBinner g_hipBinner;
extern "C" unsigned long long rdx_debug_gpu_bin_calls(void) { return g_hipBinner.calls.load(); }

extern "C" int rdx_init(int device)
{
    if (g0.initialized) return 0;
    int count = 0;
    hipError_t e = hipGetDeviceCount(&count);
    if (e != hipSuccess || count == 0)
        return fail("no HIP device available (hipGetDeviceCount -> %d, count %d): the ray-tracing core needs a GPU", (int)e, count);
    if (device < 0) { HIP_OK(hipGetDevice(&device)); }
    if (device >= count) return fail("device ordinal %d out of range (%d devices)", device, count);
    HIP_OK(hipSetDevice(device));
    g_phys[0] = device;
    g_ndev = 1;
    if (init_device_state(device)) return -1;
    g_hipBinner.device = device;
    set_gpu_binner(g0.gpuBuild ? &g_hipBinner : nullptr, (size_t)g0.gpuBuildMin);
    return 0;
}

// Single-process multi-device rendering (SURVEY 8b "Threading", 8e): after this call every buffer lives on all `n` devices
// (writes are replicated, reads come from device 0) and rdx_trace_rays renders the frame sharded by interleaved 64x64 tiles --
// one internal host thread per device, the caller still makes one blocking call -- then gathers RGBA8 and imageScratch tiles
// to device 0 with peer copies.  ordinals[i] = HIP device of logical device i (NULL: 0..n-1); logical device 0 is the one
// rdx_init chose.  Must be called before any buffer is created.  RDX_ALLOW_VIRTUAL_DEVICES=1 lets several logical devices
// share one GPU (rehearsal on a 1-GPU box; results are identical by construction).
extern "C" int rdx_init_devices(uint32_t n, const int* ordinals)
{
    if (!g0.initialized && rdx_init(ordinals ? ordinals[0] : -1)) return -1;
    if (n == 0 || n > (uint32_t)RDX_MAX_DEVICES) return fail("rdx_init_devices: %u devices (1..%d supported)", n, RDX_MAX_DEVICES);
    if (g_ndev > 1) return (uint32_t)g_ndev == n ? 0 : fail("rdx_init_devices: already initialised with %d devices", g_ndev);
    if (n == 1) return 0;
    if (!g0.buffers.empty()) return fail("rdx_init_devices must be called before any buffer is created");
    for (auto& sh : g0.shaders)
        if (sh->program) return fail("rdx_init_devices must be called before a user shader program is compiled (its code object is loaded on device 0 only)");
    int count = 0;
    HIP_OK(hipGetDeviceCount(&count));
    const bool virt = std::getenv("RDX_ALLOW_VIRTUAL_DEVICES") && std::atoi(std::getenv("RDX_ALLOW_VIRTUAL_DEVICES")) != 0;
    for (uint32_t d = 1; d < n; ++d) {
        int phys = ordinals ? ordinals[d] : (int)((g_phys[0] + d) % (uint32_t)count);
        if (phys < 0 || phys >= count) return fail("rdx_init_devices: HIP device %d does not exist (%d devices)", phys, count);
        for (uint32_t e = 0; e < d && !virt; ++e)
            if (g_phys[e] == phys) return fail("rdx_init_devices: %u devices requested, %d present (set RDX_ALLOW_VIRTUAL_DEVICES=1 to let logical devices share a GPU)", n, count);
        g_phys[d] = phys;
    }
    for (uint32_t d = 1; d < n; ++d) {
        g_dev[d] = new Context();
        tl_ctx = g_dev[d]; tl_dev = (int)d;
        hipError_t e = hipSetDevice(g_phys[d]);
        int rc = e == hipSuccess ? init_device_state(g_phys[d]) : -1;
        if (rc == 0 && g_phys[d] != g_phys[0]) {
            int can = 0;
            if (hipDeviceCanAccessPeer(&can, g_phys[0], g_phys[d]) == hipSuccess && can) {
                HIP_IGN(hipSetDevice(g_phys[0])); HIP_IGN(hipDeviceEnablePeerAccess(g_phys[d], 0)); (void)hipGetLastError();
            }
        }
        std::string msg = g.err;
        tl_ctx = &g0; tl_dev = 0;
        HIP_IGN(hipSetDevice(g_phys[0]));
        if (rc) {
            // give back what was set up so far: contexts 1..d (the failing one holds whatever its init got to)
            for (uint32_t e = 1; e <= d; ++e) {
                tl_ctx = g_dev[e]; tl_dev = (int)e;
                HIP_IGN(hipSetDevice(g_phys[e]));
                g.initialized = true;          // release_device_state frees the non-null members
                release_device_state();
                tl_ctx = &g0; tl_dev = 0;
                delete g_dev[e]; g_dev[e] = nullptr;
            }
            HIP_IGN(hipSetDevice(g_phys[0]));
            return fail("rdx_init_devices: device %u (HIP %d): %s", d, g_phys[d], msg.c_str());
        }
    }
    g_ndev = (int)n;
    return 0;
}

extern "C" int rdx_device_count(void) { return g_ndev; }

extern "C" int rdx_shutdown(void)
{
    if (!g0.initialized) return 0;
    for (int d = 1; d < g_ndev; ++d) {
        tl_ctx = g_dev[d]; tl_dev = d;
        HIP_IGN(hipSetDevice(g_phys[d]));
        for (auto& b : g0.buffers) { if (b->accelRep[d]) b->accelRep[d]->release(); if (b->rep[d]) HIP_IGN(hipFree(b->rep[d])); }
        release_device_state();
        tl_ctx = &g0; tl_dev = 0;
        delete g_dev[d];
        g_dev[d] = nullptr;
    }
    g_ndev = 1;
    HIP_IGN(hipSetDevice(g_phys[0]));
    set_gpu_binner(nullptr, 0);
    g_hipBinner.shutdown();
    HIP_IGN(hipStreamSynchronize(g.stream));
    for (auto& b : g.buffers) { if (b->accel) b->accel->release(); if (b->owned && b->dptr) HIP_IGN(hipFree(b->dptr)); }
    {   // (modules created from the same text share one compiled program: user_shader.cpp's cache)
        std::vector<UserProgram*> seen;
        for (auto& sh : g.shaders)
            if (sh->program && std::find(seen.begin(), seen.end(), sh->program) == seen.end()) { seen.push_back(sh->program); release_user_shader(sh->program); }
    }
    g.buffers.clear(); g.blases.clear(); g.shaders.clear();
    release_device_state();
    g = Context{};
    return 0;
}

extern "C" const char* rdx_last_error(void) { return g.err.c_str(); }

extern "C" int rdx_device_name(char* out, size_t cap)
{
    if (!g.initialized) return fail("rdx_init has not been called");
    hipDeviceProp_t p;
    HIP_OK(hipGetDeviceProperties(&p, g.device));
    snprintf(out, cap, "%s (%s, %d CUs)", p.name, p.gcnArchName, p.multiProcessorCount);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// buffers
// ------------------------------------------------------------------------------------------------
extern "C" rdx_buffer rdx_buffer_create(size_t size)
{
    if (!g.initialized) { fail("rdx_init has not been called"); return nullptr; }
    auto b = std::make_unique<rdx_buffer_s>();
    b->size = size;
    HIP_OKP(hipMalloc(&b->dptr, std::max<size_t>(size, 16)));
    HIP_OKP(hipMemset(b->dptr, 0, std::max<size_t>(size, 16)));
    for (int d = 1; d < g_ndev; ++d) {          // multi-device mode: one copy per device
        HIP_OKP(hipSetDevice(g_phys[d]));
        hipError_t e = hipMalloc(&b->rep[d], std::max<size_t>(size, 16));
        if (e == hipSuccess) e = hipMemset(b->rep[d], 0, std::max<size_t>(size, 16));
        HIP_IGN(hipSetDevice(g_phys[0]));
        HIP_OKP(e);
    }
    g.buffers.push_back(std::move(b));
    return g.buffers.back().get();
}

// ---- texture arrays and samplers: replaces CreateImageArray / CreateSampler / ReadImage / WriteImage
//      (radiance/src/radiance.cpp:96-137, 202-224): a 2D image array of CL_RGBA / CL_UNSIGNED_INT8 texels, layer-major
extern "C" rdx_buffer rdx_image_array_create(uint32_t width, uint32_t height, uint32_t layers)
{
    if ((uint64_t)width * height * std::max(layers, 1u) * 4ull > (1ull << 36)) { fail("CreateImageArray: %ux%ux%u is too large", width, height, layers); return nullptr; }
    rdx_buffer b = rdx_buffer_create((size_t)width * height * layers * 4);
    if (!b) return nullptr;
    b->imgW = width; b->imgH = height; b->imgLayers = layers;
    return b;
}

static int image_region(rdx_buffer img, uint32_t width, uint32_t height, size_t layer, const char* what)
{
    if (!img || !known_buffer(img) || !img->imgW) return fail("%s: not an image array", what);
    if (layer >= img->imgLayers) return fail("%s: layer %zu of %u", what, layer, img->imgLayers);
    if (width > img->imgW || height > img->imgH) return fail("%s: region %ux%u exceeds the image (%ux%u)", what, width, height, img->imgW, img->imgH);
    return 0;
}

// origin (0, 0, layer), region (width, height, 1), host rows tightly packed -- as radiance.cpp:202-224 calls clEnqueue{Write,Read}Image
extern "C" int rdx_image_write(rdx_buffer img, uint32_t width, uint32_t height, size_t layer, const void* rgba8)
{
    if (image_region(img, width, height, layer, "WriteImage")) return -1;
    if (!width || !height) return 0;
    uint8_t* dst = static_cast<uint8_t*>(img->dptr) + layer * (size_t)img->imgW * img->imgH * 4;
    HIP_OK(hipMemcpy2D(dst, (size_t)img->imgW * 4, rgba8, (size_t)width * 4, (size_t)width * 4, height, hipMemcpyHostToDevice));
    for (int d = 1; d < g_ndev; ++d) {
        HIP_OK(hipSetDevice(g_phys[d]));
        hipError_t e = hipMemcpy2D(static_cast<uint8_t*>(img->rep[d]) + layer * (size_t)img->imgW * img->imgH * 4, (size_t)img->imgW * 4, rgba8,
                                   (size_t)width * 4, (size_t)width * 4, height, hipMemcpyHostToDevice);
        HIP_IGN(hipSetDevice(g_phys[0]));
        HIP_OK(e);
    }
    ++img->version;
    return 0;
}

extern "C" int rdx_image_read(rdx_buffer img, uint32_t width, uint32_t height, size_t layer, void* rgba8)
{
    if (image_region(img, width, height, layer, "ReadImage")) return -1;
    if (!width || !height) return 0;
    const uint8_t* src = static_cast<const uint8_t*>(img->dptr) + layer * (size_t)img->imgW * img->imgH * 4;
    HIP_OK(hipMemcpy2D(rgba8, (size_t)width * 4, src, (size_t)img->imgW * 4, (size_t)width * 4, height, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" rdx_sampler rdx_sampler_create(uint32_t addressingMode, uint32_t filterMode)
{
    if (addressingMode < 0x1131 || addressingMode > 0x1134 || (filterMode != 0x1140 && filterMode != 0x1141)) {
        fail("CreateSampler: addressing mode 0x%x / filter mode 0x%x are not CL_ADDRESS_* / CL_FILTER_* values", addressingMode, filterMode);
        return nullptr;
    }
    auto sm = std::make_unique<rdx_sampler_s>();
    sm->addressing = addressingMode; sm->filter = filterMode;
    g.samplers.push_back(std::move(sm));
    return g.samplers.back().get();
}

extern "C" rdx_buffer rdx_buffer_wrap(void* device_ptr, size_t size)
{
    if (!g.initialized) { fail("rdx_init has not been called"); return nullptr; }
    if (!device_ptr) { fail("rdx_buffer_wrap: null device pointer"); return nullptr; }
    auto b = std::make_unique<rdx_buffer_s>();
    if (g_ndev > 1) { fail("rdx_buffer_wrap: caller-owned device memory cannot be replicated in multi-device mode"); return nullptr; }
    b->size = size; b->dptr = device_ptr; b->owned = false;
    g.buffers.push_back(std::move(b));
    return g.buffers.back().get();
}

extern "C" int rdx_buffer_write(rdx_buffer b, size_t offset, size_t size, const void* src)
{
    if (!b || !known_buffer(b)) return fail("WriteBuffer: invalid buffer handle");
    if (offset + size > b->size) return fail("WriteBuffer: range [%zu, %zu) exceeds buffer size %zu", offset, offset + size, b->size);
    if (size) HIP_OK(hipMemcpy(static_cast<uint8_t*>(b->dptr) + offset, src, size, hipMemcpyHostToDevice));
    for (int d = 1; d < g_ndev && size; ++d) {   // replicate
        HIP_OK(hipSetDevice(g_phys[d]));
        hipError_t e = hipMemcpy(static_cast<uint8_t*>(b->rep[d]) + offset, src, size, hipMemcpyHostToDevice);
        HIP_IGN(hipSetDevice(g_phys[0]));
        HIP_OK(e);
    }
    b->version++;
    if (b->owned && b->size <= 256) {
        if (offset == 0 && size == b->size) { b->mirror.assign(static_cast<const uint8_t*>(src), static_cast<const uint8_t*>(src) + size); b->mirrorValid = true; }
        else if (b->mirrorValid && size) std::memcpy(b->mirror.data() + offset, src, size);
    }
    return 0;
}

extern "C" int rdx_buffer_read(rdx_buffer b, size_t offset, size_t size, void* dst)
{
    if (!b || !known_buffer(b)) return fail("ReadBuffer: invalid buffer handle");
    if (offset + size > b->size) return fail("ReadBuffer: range [%zu, %zu) exceeds buffer size %zu", offset, offset + size, b->size);
    HIP_OK(hipStreamSynchronize(g.stream));
    if (size) HIP_OK(hipMemcpy(dst, static_cast<const uint8_t*>(b->dptr) + offset, size, hipMemcpyDeviceToHost));
    return 0;
}

extern "C" void* rdx_buffer_device_ptr(rdx_buffer b) { return (b && known_buffer(b)) ? b->dptr : nullptr; }
extern "C" size_t rdx_buffer_size(rdx_buffer b) { return (b && known_buffer(b)) ? b->size : 0; }

// ------------------------------------------------------------------------------------------------
// acceleration structures
// ------------------------------------------------------------------------------------------------
extern "C" rdx_blas rdx_blas_build(const float* v, uint32_t nv, const uint32_t* idx, uint32_t nt)
{
    std::string err;
    Blas* b = build_blas(v, nv, idx, nt, err);
    if (!b) { fail("%s", err.c_str()); return nullptr; }
    auto h = std::make_unique<rdx_blas_s>();
    h->blas.reset(b);
    g.blases.push_back(std::move(h));
    return g.blases.back().get();
}

// Several meshes at once: the builds are independent (one BVH per mesh), so they run on a pool of host threads inside the
// library -- the caller stays single-threaded (radiance.h has no such call; the reference builds its meshes one after the
// other, tools/sceneBuilder.cpp:229-258).  Results are identical to `count` rdx_blas_build calls in order.
extern "C" int rdx_blas_build_many(uint32_t count, const float* const* verts, const uint32_t* nverts,
                                   const uint32_t* const* indices, const uint32_t* ntris, rdx_blas* out)
{
    if (count == 0) return 0;
    if (!verts || !nverts || !indices || !ntris || !out) return fail("rdx_blas_build_many: null argument");
    std::vector<Blas*> built(count, nullptr);
    std::vector<std::string> errs(count);
    std::atomic<uint32_t> next{0};
    const uint32_t nthreads = std::max(1u, std::min(count, std::min(16u, std::thread::hardware_concurrency())));
    auto work = [&]() {
        for (;;) {
            const uint32_t i = next.fetch_add(1);
            if (i >= count) return;
            built[i] = build_blas(verts[i], nverts[i], indices[i], ntris[i], errs[i]);
        }
    };
    std::vector<std::thread> pool;
    for (uint32_t t = 1; t < nthreads; ++t) pool.emplace_back(work);
    work();
    for (auto& t : pool) t.join();
    for (uint32_t i = 0; i < count; ++i)
        if (!built[i]) {
            for (Blas* b : built) delete b;
            return fail("mesh %u: %s", i, errs[i].c_str());
        }
    for (uint32_t i = 0; i < count; ++i) {
        auto h = std::make_unique<rdx_blas_s>();
        h->blas.reset(built[i]);
        g.blases.push_back(std::move(h));
        out[i] = g.blases.back().get();
    }
    return 0;
}

extern "C" const void* rdx_blas_data(rdx_blas b, uint32_t* size_out)
{
    if (!b) return nullptr;
    if (size_out) *size_out = (uint32_t)b->blas->data.size();
    return b->blas->data.data();
}
extern "C" int rdx_blas_max_depth(rdx_blas b) { return b ? b->blas->maxDepth : -1; }

static rdx_buffer tlas_from_blob(std::vector<uint8_t>&& blob)
{
    rdx_buffer tb = rdx_buffer_create(blob.size());
    if (!tb) return nullptr;
    if (rdx_buffer_write(tb, 0, blob.size(), blob.data()) != 0) return nullptr;
    tb->shadow = std::move(blob);
    tb->shadowVersion = tb->version;
    return tb;
}

static bool tlas_blob(const rdx_instance* inst, uint32_t n, std::vector<uint8_t>& blob, int& depth, bool topOnly = false)
{
    std::vector<InstanceDesc> d(n);
    for (uint32_t i = 0; i < n; ++i) {
        std::memcpy(d[i].transform, inst[i].transform, 64);
        d[i].SBTOffset = inst[i].SBTOffset;
        d[i].customInstanceID = inst[i].customInstanceID;
        d[i].blas = inst[i].bottomAccelStruct ? inst[i].bottomAccelStruct->blas.get() : nullptr;
    }
    std::string err;
    if (!(topOnly ? build_tlas_top(d.data(), n, blob, depth, err) : build_tlas(d.data(), n, blob, depth, err))) { fail("%s", err.c_str()); return false; }
    return true;
}

extern "C" void* rdx_tlas_build_blob(const rdx_instance* inst, uint32_t n, uint32_t* size_out, int* max_depth_out)
{
    std::vector<uint8_t> blob;
    int depth = 0;
    if (!tlas_blob(inst, n, blob, depth)) return nullptr;
    void* p = malloc(blob.size());
    if (!p) { fail("out of memory"); return nullptr; }
    std::memcpy(p, blob.data(), blob.size());
    if (size_out) *size_out = (uint32_t)blob.size();
    if (max_depth_out) *max_depth_out = depth;
    return p;
}
extern "C" void rdx_free(void* p) { free(p); }

extern "C" rdx_buffer rdx_tlas_build(const rdx_instance* inst, uint32_t n)
{
    if (!g.initialized) { fail("rdx_init has not been called"); return nullptr; }
    std::vector<uint8_t> blob;
    int depth = 0;
    if (!tlas_blob(inst, n, blob, depth)) return nullptr;
    rdx_buffer tb = tlas_from_blob(std::move(blob));
    if (tb) for (uint32_t i = 0; i < n; ++i) tb->tlasBlas.push_back(inst[i].bottomAccelStruct);
    return tb;
}

// ---- rdx_tlas_update ---------------------------------------------------------------------------------------------------------
// The blob of other transforms differs from the one in the buffer in its top part only -- header, top-level nodes, instance
// records; the BLAS region behind them is byte-identical and merely shifts when the number of top-level nodes changes
// (build_tlas appends the distinct BLASes in order of first appearance by instance INDEX, which an update keeps).  So: the top
// part is built by the builder (build_tlas_top) and uploaded; a shifted region is copied on the device into a buffer of the new
// size, and the old buffer freed.  A traversal layout that was derived for the old blob follows by update_accel_layout: the small
// arrays are uploaded again, the triangle owner words rewritten by one kernel, and nothing else moves.
namespace {
// the layout part of the update for the calling thread's device (tl_ctx / tl_dev, HIP device current); `oldVersion`: what the
// cache must have been derived from to be updated rather than left for the next derive_accel
int update_accel(rdx_buffer_s* tb, uint64_t oldVersion, rdx_tlas_update_stats& st)
{
    AccelCache* ac = acc(tb).get();
    if (!ac || ac->version != oldVersion) return 0;
    AccelUpdate upd;
    std::string err;
    const uint32_t topBefore = (uint32_t)ac->host.tnodes.size();
    int rc = update_accel_layout(tb->shadow.data(), tb->shadow.size(), AccelOptions{g.opt.quad, g.opt.cull}, ac->host, upd, err);
    if (rc < 0) return fail_str(err);
    uint64_t total = 0;
    for (const AccelOwnerRange& r : upd.owners) {
        if ((uint64_t)r.first + r.count > ac->host.book.nTris) return fail("rdx_tlas_update: owner range [%u, +%u) beyond %u triangle slots", r.first, r.count, ac->host.book.nTris);
        total += r.count;
    }
    if (rc == 0 && (ac->host.tnodes.size() > ac->topCap || (size_t)upd.wideTailFirst + upd.wideTail.size() > ac->wideCap || total > 0xffffffffull)) rc = 1;
    if (rc == 1) {                  // the full derivation (it replaces the cache: nothing of the old one is kept)
        st.path = 2;
        st.top_nodes_before = topBefore;
        if (derive_accel(tb)) return -1;
        st.top_nodes_after = (uint32_t)acc(tb)->host.tnodes.size();
        return 0;
    }
    st.path = std::max(st.path, 1u);
    st.top_nodes_before = topBefore; st.top_nodes_after = (uint32_t)ac->host.tnodes.size();
    const AccelLayout& L = ac->host;
    auto h2d = [&](void* dst, const void* src, size_t bytes) -> hipError_t {
        st.bytes_h2d += bytes;
        return bytes ? hipMemcpyAsync(dst, src, bytes, hipMemcpyHostToDevice, g.stream) : hipSuccess;
    };
    if (upd.tnodes) HIP_OK(h2d(ac->tnodes, L.tnodes.data(), L.tnodes.size() * sizeof(DNode)));
    if (upd.ctnodes) HIP_OK(h2d(ac->ctnodes, L.ctnodes.data(), L.ctnodes.size() * sizeof(DNode)));
    const std::vector<uint32_t> slots = slot_table(L.insts);        // (lives until the synchronisation below)
    if (upd.insts) {
        HIP_OK(h2d(ac->insts, L.insts.data(), L.insts.size() * sizeof(DInst)));
        HIP_OK(h2d(ac->slotOf, slots.data(), slots.size() * sizeof(uint32_t)));     // another top-level tree orders the slots anew
    }
    if (upd.groupBits) HIP_OK(h2d(ac->groupBits, L.groupBits, sizeof L.groupBits));
    if (upd.entries && ac->entriesUp) HIP_OK(h2d(ac->quad + ac->nQuad, L.entries.data(), L.entries.size() * sizeof(DQuad)));   // (same count: one per slot)
    if (upd.wideTailChanged) HIP_OK(h2d(ac->wide + upd.wideTailFirst, upd.wideTail.data(), upd.wideTail.size() * sizeof(DWide)));
    std::vector<uint4> table;
    if (!upd.owners.empty()) {
        uint32_t before = 0;
        for (const AccelOwnerRange& r : upd.owners) { table.push_back(uint4{r.first, r.count, r.owner, before}); before += r.count; }
        if (table.size() > ac->ownerCap) {
            if (ac->ownerTable) HIP_IGN(hipFree(ac->ownerTable));
            ac->ownerTable = nullptr; ac->ownerCap = 0;
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&ac->ownerTable), std::max<size_t>(table.size(), L.book.blocks.size()) * sizeof(uint4)));
            ac->ownerCap = std::max<size_t>(table.size(), L.book.blocks.size());
        }
        HIP_OK(h2d(ac->ownerTable, table.data(), table.size() * sizeof(uint4)));
        HIP_OK(hipEventRecord(g.evA, g.stream));
        launch_tri_owner_fill(g.stream, ac->tris, L.book.nTris, ac->ownerTable, (uint32_t)table.size(), (uint32_t)total);
        HIP_OK(hipEventRecord(g.evB, g.stream));
        HIP_OK(hipGetLastError());
    }
    HIP_OK(hipStreamSynchronize(g.stream));          // (the host arrays above go out of scope / may change with the next update)
    if (!table.empty()) { float ms = 0; HIP_OK(hipEventElapsedTime(&ms, g.evA, g.evB)); st.ms_device += ms; }
    st.tri_slots_rewritten += total;
    ac->s = L.s;
    ac->s.coopOK = runtime_coop_ok(L.s);
    ac->version = tb->version;
    return 0;
}
}

extern "C" int rdx_tlas_update(rdx_buffer tb, const rdx_instance* inst, uint32_t n)
{
    if (!g0.initialized) return fail("rdx_init has not been called");
    if (!tb || !known_buffer(tb)) return fail("rdx_tlas_update: invalid TLAS handle");
    if (!tb->owned || tb->tlasBlas.empty()) return fail("rdx_tlas_update: the buffer is not a TLAS built by rdx_tlas_build (wrapped memory, a cache file and plain buffers cannot be updated)");
    if (tb->shadowVersion != tb->version) return fail("rdx_tlas_update: the TLAS buffer has been written to since it was built");
    if (!inst) return fail("rdx_tlas_update: no instances");
    if (n != tb->tlasBlas.size()) return fail("rdx_tlas_update: %u instances, the TLAS was built from %zu", n, tb->tlasBlas.size());
    for (uint32_t i = 0; i < n; ++i)       // (handles are compared, not followed: BLAS handles live until rdx_shutdown)
        if (inst[i].bottomAccelStruct != tb->tlasBlas[i]) return fail("rdx_tlas_update: instance %u refers to another BLAS than the TLAS was built with", i);
    const auto t0 = std::chrono::steady_clock::now();
    std::vector<uint8_t> top;
    int depth = 0;
    if (!tlas_blob(inst, n, top, depth, true)) return -1;
    const auto* oh = reinterpret_cast<const BlobTopHeader*>(tb->shadow.data());
    const size_t oldTop = (size_t)oh->instByteOffset + (size_t)n * sizeof(BlobInst), newTop = top.size();
    if (oldTop > tb->shadow.size()) return fail("rdx_tlas_update: the TLAS blob is malformed");
    const size_t region = tb->shadow.size() - oldTop, newSize = newTop + region, oldSize = tb->size;
    if (reinterpret_cast<const BlobTopHeader*>(top.data())->totalBufferSize != newSize) return fail("rdx_tlas_update: the builder's top part does not fit the BLAS region");

    rdx_tlas_update_stats st{};
    // the blob on every device
    for (int d = 0; d < g_ndev; ++d) {
        void*& ptr = d == 0 ? tb->dptr : tb->rep[d];
        HIP_OK(hipSetDevice(g_phys[d]));
        hipError_t e = hipSuccess;
        if (newTop == oldTop) e = hipMemcpy(ptr, top.data(), newTop, hipMemcpyHostToDevice);
        else {
            // the region moves: into a second allocation (an overlapping copy inside one buffer is not defined), the old one is freed
            void* fresh = nullptr;
            e = hipMalloc(&fresh, std::max<size_t>(newSize, 16));
            if (e == hipSuccess) e = hipMemcpy(fresh, top.data(), newTop, hipMemcpyHostToDevice);
            if (e == hipSuccess && region) e = hipMemcpy(static_cast<uint8_t*>(fresh) + newTop, static_cast<const uint8_t*>(ptr) + oldTop, region, hipMemcpyDeviceToDevice);
            if (e == hipSuccess) e = hipDeviceSynchronize();
            if (e == hipSuccess) { HIP_IGN(hipFree(ptr)); ptr = fresh; st.bytes_d2d += region; }
            else if (fresh) HIP_IGN(hipFree(fresh));
        }
        HIP_IGN(hipSetDevice(g_phys[0]));
        HIP_OK(e);
        st.bytes_h2d += newTop;
    }
    // the host shadow, kept equal to the device blob without reading it back
    if (newTop < oldTop) { std::memmove(tb->shadow.data() + newTop, tb->shadow.data() + oldTop, region); tb->shadow.resize(newSize); }
    else if (newTop > oldTop) { tb->shadow.resize(newSize); std::memmove(tb->shadow.data() + newTop, tb->shadow.data() + oldTop, region); }
    std::memcpy(tb->shadow.data(), top.data(), newTop);
    (void)oldSize;
    tb->size = newSize;
    const uint64_t oldVersion = tb->version++;
    tb->shadowVersion = tb->version;
    st.top_nodes_before = (uint32_t)((oldTop - (size_t)n * sizeof(BlobInst) - 16) / sizeof(BlobNode));
    st.top_nodes_after = (uint32_t)((newTop - (size_t)n * sizeof(BlobInst) - 16) / sizeof(BlobNode));
    const auto t1 = std::chrono::steady_clock::now();
    // the traversal layout on every device that had derived one
    for (int d = 0; d < g_ndev; ++d) {
        if (d) g_dev[d]->opt = g0.opt;
        tl_ctx = g_dev[d]; tl_dev = d;
        hipError_t e = hipSetDevice(g_phys[d]);
        const int rc = e == hipSuccess ? update_accel(tb, oldVersion, st) : -1;
        const std::string msg = g.err;
        tl_ctx = &g0; tl_dev = 0;
        HIP_IGN(hipSetDevice(g_phys[0]));
        if (rc) return fail("rdx_tlas_update: device %d: %s", d, e == hipSuccess ? msg.c_str() : hipGetErrorString(e));
    }
    const auto t2 = std::chrono::steady_clock::now();
    (void)t1;
    st.ms_host = std::chrono::duration<float, std::milli>(t2 - t0).count() - st.ms_device;
    g0.updStats = st;
    return 0;
}

extern "C" int rdx_get_tlas_update_stats(rdx_tlas_update_stats* out)
{
    if (!out) return fail("rdx_get_tlas_update_stats: null argument");
    *out = g0.updStats;
    return 0;
}

// radiance.cpp:428-448: raw dump of the TLAS buffer, size from header word 3
// error text set from the library's other translation units (scene_obj.cpp)
namespace rdx { int fail_text(const char* text) { return fail_str(text ? text : ""); } }

// Side-car of a TLAS cache file: the cache itself stays the raw blob the reference writes
// (radiance.cpp:428-448: totalBufferSize bytes, no header of its own), so files written by either side load on the
// other; `<path>.meta` adds what the raw format cannot say -- a magic / version line, the byte count and an FNV-1a
// hash of the blob.  FileToTopAccelStruct verifies a side-car when one exists and refuses a blob that does not
// match it (a truncated or stale cache is otherwise only noticed as a wrong picture); a cache without side-car
// loads as before.
static uint64_t fnv1a64(const uint8_t* p, size_t n)
{
    uint64_t h = 1469598103934665603ull;
    for (size_t i = 0; i < n; ++i) { h ^= p[i]; h *= 1099511628211ull; }
    return h;
}
static int write_cache_meta(const char* path, const std::vector<uint8_t>& data)
{
    const std::string mp = std::string(path) + ".meta";
    FILE* fp = fopen(mp.c_str(), "w");
    if (!fp) return fail("TopAccelStructToFile: cannot open '%s' for writing", mp.c_str());
    const int ok = fprintf(fp, "RDXCACHE 1\nbytes %zu\nfnv1a64 %016llx\n", data.size(), (unsigned long long)fnv1a64(data.data(), data.size()));
    fclose(fp);
    return ok > 0 ? 0 : fail("TopAccelStructToFile: short write to '%s'", mp.c_str());
}
// 0 = no side-car or it matches, -1 = mismatch (error text set)
static int check_cache_meta(const char* path, const std::vector<uint8_t>& data)
{
    const std::string mp = std::string(path) + ".meta";
    FILE* fp = fopen(mp.c_str(), "r");
    if (!fp) return 0;
    char magic[16] = ""; int ver = 0; size_t bytes = 0; unsigned long long h = 0;
    const int n = fscanf(fp, "%15s %d bytes %zu fnv1a64 %llx", magic, &ver, &bytes, &h);
    fclose(fp);
    if (n != 4 || strcmp(magic, "RDXCACHE")) return fail("FileToTopAccelStruct: '%s' is not a cache side-car", mp.c_str());
    if (ver != 1) return fail("FileToTopAccelStruct: side-car '%s' has version %d, this library reads version 1", mp.c_str(), ver);
    if (bytes != data.size()) return fail("FileToTopAccelStruct: '%s' holds %zu bytes, its side-car says %zu (stale or truncated cache)", path, data.size(), bytes);
    if (h != fnv1a64(data.data(), data.size())) return fail("FileToTopAccelStruct: '%s' does not match the hash in its side-car (stale or corrupted cache)", path);
    return 0;
}

extern "C" int rdx_tlas_to_file(rdx_buffer tlas, const char* path)
{
    if (!tlas || !known_buffer(tlas)) return fail("TopAccelStructToFile: invalid handle");
    BlobTopHeader hdr;
    if (rdx_buffer_read(tlas, 0, sizeof hdr, &hdr)) return -1;
    if (hdr.totalBufferSize > tlas->size) return fail("TopAccelStructToFile: header size %u exceeds buffer size %zu", hdr.totalBufferSize, tlas->size);
    std::vector<uint8_t> data(hdr.totalBufferSize);
    if (rdx_buffer_read(tlas, 0, data.size(), data.data())) return -1;
    FILE* fp = fopen(path, "wb");
    if (!fp) return fail("TopAccelStructToFile: cannot open '%s' for writing", path);
    const size_t wr = fwrite(data.data(), 1, data.size(), fp);
    fclose(fp);
    if (wr != data.size()) return fail("TopAccelStructToFile: short write to '%s'", path);
    return write_cache_meta(path, data);
}

// radiance.cpp:450-479
extern "C" rdx_buffer rdx_tlas_from_file(const char* path)
{
    if (!g.initialized) { fail("rdx_init has not been called"); return nullptr; }
    FILE* fp = fopen(path, "rb");
    if (!fp) { fail("FileToTopAccelStruct: cannot open '%s'", path); return nullptr; }
    BlobTopHeader hdr;
    if (fread(&hdr, 1, sizeof hdr, fp) != sizeof hdr) { fclose(fp); fail("FileToTopAccelStruct: short read of header in '%s'", path); return nullptr; }
    if (hdr.type != TYPE_TOP_AS || hdr.totalBufferSize < sizeof hdr) { fclose(fp); fail("FileToTopAccelStruct: '%s' is not a TLAS cache file", path); return nullptr; }
    std::vector<uint8_t> data(hdr.totalBufferSize);
    rewind(fp);
    const size_t rd = fread(data.data(), 1, data.size(), fp);
    fclose(fp);
    if (rd != data.size()) { fail("FileToTopAccelStruct: short read of '%s' (%zu of %zu bytes)", path, rd, data.size()); return nullptr; }
    if (check_cache_meta(path, data)) return nullptr;
    return tlas_from_blob(std::move(data));
}

// ------------------------------------------------------------------------------------------------
// pipeline
// ------------------------------------------------------------------------------------------------
static bool has_identifier(const std::string& text, const char* name)
{
    const size_t n = strlen(name);
    size_t pos = 0;
    auto isid = [](char c) { return (c >= 'a' && c <= 'z') || (c >= 'A' && c <= 'Z') || (c >= '0' && c <= '9') || c == '_'; };
    while ((pos = text.find(name, pos)) != std::string::npos) {
        const bool l = pos == 0 || !isid(text[pos - 1]);
        const bool r = pos + n >= text.size() || !isid(text[pos + n]);
        if (l && r) return true;
        pos += n;
    }
    return false;
}

// text with comments removed (so that a commented-out parameter list or identifier does not count)
static std::string strip_comments(const std::string& t)
{
    std::string o;
    o.reserve(t.size());
    for (size_t i = 0; i < t.size();) {
        if (t.compare(i, 2, "//") == 0) {
            // to the end of the line -- of the LOGICAL line: a backslash in front of the newline continues the comment, as it does
            // for the compiler (the newlines stay, for the line numbers)
            for (; i < t.size(); ++i) {
                if (t[i] != '\n') continue;
                size_t b = i;
                if (b > 0 && t[b - 1] == '\r') --b;
                if (b > 0 && t[b - 1] == '\\') { o.push_back('\n'); continue; }
                break;
            }
        }
        else if (t.compare(i, 2, "/*") == 0) { const size_t e = t.find("*/", i + 2); const size_t j = e == std::string::npos ? t.size() : e + 2; o.push_back(' '); for (; i < j; ++i) if (t[i] == '\n') o.push_back('\n'); }
        else o.push_back(t[i++]);
    }
    return o;
}

// does `raygen` take parameters?  (-1: no raygen( found)
static int raygen_has_parameters(const std::string& t)
{
    for (size_t pos = t.find("raygen"); pos != std::string::npos; pos = t.find("raygen", pos + 1)) {
        size_t i = pos + 6;
        while (i < t.size() && std::isspace((unsigned char)t[i])) ++i;
        if (i >= t.size() || t[i] != '(') continue;
        const size_t e = t.find(')', i);
        if (e == std::string::npos) return -1;
        std::string inner = t.substr(i + 1, e - i - 1);
        inner.erase(std::remove_if(inner.begin(), inner.end(), [](unsigned char c) { return std::isspace(c); }), inner.end());
        return (inner.empty() || inner == "void") ? 0 : 1;
    }
    return -1;
}

static uint64_t fnv1a64_nows(const std::string& t)
{
    uint64_t h = 0xcbf29ce484222325ull;
    for (unsigned char c : t) { if (std::isspace(c)) continue; h ^= c; h *= 0x100000001b3ull; }
    return h;
}

// A program text with the BODIES of its closest-hit / miss stage functions blanked out (the functions sbt.json names for rows
// without an any-hit shader, and the miss rows): two programs that agree on it differ only inside those functions -- the raygen
// loop, the payload / scene structs, the helper functions, the any-hit rows and the dispatch tables are the same.
// What blank_bodies does beyond blanking when it makes the REDUCED text of the eligibility rule (blank_stage_bodies).
struct ReducedText {
    bool lasting = false;       // out: a blanked body holds a preprocessor directive that outlives the function
};
// A directive that outlives the function it stands in: anything but #include and the conditionals (#if / #ifdef / #ifndef /
// #elif / #else / #endif) -- #define, #undef, #pragma, #line ..., spelled `#` or with the digraph `%:` -- and the _Pragma
// operator anywhere in the body.  The text behind such a body no longer means what the same characters mean in the stock program.
static bool body_has_lasting_directive(const std::string& t, size_t from, size_t to)
{
    static const char* const kLocal[] = {"include", "if", "ifdef", "ifndef", "elif", "else", "endif"};
    auto ident = [](char c) { return std::isalnum((unsigned char)c) || c == '_'; };
    bool lineStart = true;
    for (size_t i = from; i < to; ++i) {
        const char c = t[i];
        if (c == '\n') { lineStart = true; continue; }
        if (c == ' ' || c == '\t' || c == '\r') continue;
        const bool digraph = c == '%' && i + 1 < to && t[i + 1] == ':';
        if (lineStart && (c == '#' || digraph)) {
            size_t a = i + (digraph ? 2 : 1);
            while (a < to && (t[a] == ' ' || t[a] == '\t')) ++a;
            size_t b = a;
            while (b < to && ident(t[b])) ++b;
            const std::string word = t.substr(a, b - a);
            bool local = word.empty();                         // a null directive
            for (const char* k : kLocal) if (word == k) local = true;
            if (!local) return true;
        }
        if (t.compare(i, 7, "_Pragma") == 0 && (i == 0 || !ident(t[i - 1])) && (i + 7 >= t.size() || !ident(t[i + 7]))) return true;
        lineStart = false;
    }
    return false;
}
// does the line that holds `pos` begin with a preprocessor directive (`#` or `%:` after blanks)?
static bool on_directive_line(const std::string& t, size_t pos)
{
    size_t ls = pos;
    while (ls > 0 && t[ls - 1] != '\n') --ls;
    while (ls < pos && (t[ls] == ' ' || t[ls] == '\t')) ++ls;
    return t[ls] == '#' || (t[ls] == '%' && ls + 1 < t.size() && t[ls + 1] == ':');
}
static void blank_bodies(std::string& t, const std::vector<std::string>& names, ReducedText* reduced = nullptr)
{
    for (const std::string& fn : names) {
        size_t pos = 0;
        while ((pos = t.find(fn, pos)) != std::string::npos) {
            const size_t end = pos + fn.size();
            const bool startOK = pos == 0 || !(std::isalnum((unsigned char)t[pos - 1]) || t[pos - 1] == '_');
            size_t q = end;
            while (q < t.size() && std::isspace((unsigned char)t[q])) ++q;
            if (!startOK || q >= t.size() || t[q] != '(') { pos = end; continue; }
            // parameter list, then a definition's '{' (a call or a prototype has something else there)
            int depth = 0;
            size_t r = q;
            for (; r < t.size(); ++r) { if (t[r] == '(') ++depth; else if (t[r] == ')') { if (--depth == 0) { ++r; break; } } }
            while (r < t.size() && std::isspace((unsigned char)t[r])) ++r;
            if (reduced && r < t.size() && t[r] == ';' && !on_directive_line(t, pos) &&
                std::count(t.begin(), t.begin() + pos, '{') == std::count(t.begin(), t.begin() + pos, '}')) {
                // the reduced text only: a prototype of a stage function at file scope (a call is inside some body; the replacement
                // list of a #define is neither) declares what the definition declares anyway; it goes, back to the end of whatever
                // precedes it, never across a preprocessor line
                size_t from = pos;
                while (from > 0 && t[from - 1] != ';' && t[from - 1] != '}' && !(t[from - 1] == '\n' && on_directive_line(t, from - 1))) --from;
                std::string gap((size_t)std::count(t.begin() + from, t.begin() + r + 1, '\n'), '\n');
                t.replace(from, r + 1 - from, gap);
                pos = from + gap.size();
                continue;
            }
            if (r >= t.size() || t[r] != '{') { pos = end; continue; }
            int braces = 0;
            size_t e = r;
            for (; e < t.size(); ++e) { if (t[e] == '{') ++braces; else if (t[e] == '}') { if (--braces == 0) { ++e; break; } } }
            if (reduced && body_has_lasting_directive(t, r, e)) reduced->lasting = true;
            std::string blank = "{";
            blank.append((size_t)std::count(t.begin() + r, t.begin() + e, '\n'), '\n');       // line numbers stay (compiler diagnostics)
            blank += "}";
            t.replace(r, e - r, blank);
            pos = r + blank.size();
        }
    }
}
// -> false: the program has no reduced text -- a #define / #undef / #pragma inside a stage function reaches the text behind it,
// which a reduced text could not show; such a program is not "the stock program outside its stage functions" and runs as the
// megakernel it is.
static bool blank_stage_bodies(const std::string& text, std::string& out)
{
    std::string t = strip_comments(text);
    std::vector<std::string> names;
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
        static const Row miss[] = {
#define X(row, fn) {row, #fn},
            RDX_SBT_MISS(X)
#undef X
            {-1, nullptr}};
        for (const Row* c = closest; c->fn; ++c) {
            bool hasAny = false;
            for (const Row* a = anyHit; a->fn; ++a) if (a->row == c->row) hasAny = true;
            if (!hasAny) names.push_back(c->fn);
        }
        for (const Row* m = miss; m->fn; ++m) names.push_back(m->fn);
    }
    ReducedText reduced;
    blank_bodies(t, names, &reduced);
    out = t;
    return !reduced.lasting;
}
// the hash the eligibility rule compares with the stock program's; 0 (no program's) where there is no reduced text
static uint64_t stage_reduced_hash(const std::string& text)
{
    std::string t;
    return blank_stage_bodies(text, t) ? fnv1a64_nows(t) : 0;
}
extern "C" unsigned long long rdx_debug_stage_reduced_hash(const char* code, uint32_t size)
{
    return code ? stage_reduced_hash(std::string(code, size)) : (unsigned long long)RDX_STOCK_REDUCED_HASH;   // null: the stock program's
}

// Compile-only check of the run-time shader compiler (no device needed; the CPU suite uses it): 0 = the program compiles in
// the given mode (stages: with its raygen body blanked, as rdx_shader_module_create does), -1 = it does not, the log in the
// last-error string.  "Compiles" = every step up to loading the code object succeeded.
extern "C" int rdx_debug_jit_compiles(const char* code, uint32_t size, const char* arch, int stages)
{
    if (!code || !arch) return fail("rdx_debug_jit_compiles: null argument");
    std::string text(code, size), err;
    if (stages) { text = strip_comments(text); blank_bodies(text, {"raygen", "generateRay"}); }
    setenv("RDX_JIT_COMPILE_ONLY", "1", 1);
    UserProgram* p = compile_user_shader(text, g0.shaderInclude, arch, stages != 0, err);
    unsetenv("RDX_JIT_COMPILE_ONLY");
    (void)p;
    if (err == "compiled") return 0;
    return fail_str(err.empty() ? std::string("rdx_debug_jit_compiles: unexpected state") : err);
}

// The same, and the code object is written to `out_path` (an absolute path) for inspection -- its instructions, its kernels'
// resources -- instead of being loaded.  Programs this process already built are compiled again.
extern "C" int rdx_debug_jit_compile_to(const char* code, uint32_t size, const char* arch, int stages, const char* out_path)
{
    if (!code || !arch || !out_path || out_path[0] != '/') return fail("rdx_debug_jit_compile_to: null argument or a relative path");
    std::string text(code, size), err;
    if (stages) { text = strip_comments(text); blank_bodies(text, {"raygen", "generateRay"}); }
    setenv("RDX_JIT_COMPILE_ONLY", out_path, 1);
    UserProgram* p = compile_user_shader(text, g0.shaderInclude, arch, stages != 0, err);
    unsetenv("RDX_JIT_COMPILE_ONLY");
    (void)p;
    if (err == "compiled") return 0;
    return fail_str(err.empty() ? std::string("rdx_debug_jit_compile_to: unexpected state") : err);
}

// The run-time compiler's cache key of a program (megakernel or stage text as given): abi < 0 = this build's RDX_JIT_ABI,
// bitcode null = the library's own texture bitcode, else that file.
extern "C" unsigned long long rdx_debug_jit_key(const char* code, uint32_t size, const char* arch, int stages, int abi, const char* bitcode)
{
    if (!code || !arch) return 0;
    return (unsigned long long)user_shader_key(std::string(code, size), g0.shaderInclude, arch, stages != 0, abi < 0 ? RDX_JIT_ABI : abi,
                                               bitcode ? std::string(bitcode) : std::string());
}

extern "C" int rdx_shader_include_path(const char* path)
{
    g0.shaderInclude = path ? path : "";
    return 0;
}

extern "C" rdx_shader rdx_shader_module_create(const char* code, uint32_t size, const char* name)
{
    if (!g.initialized) { fail("rdx_init has not been called"); return nullptr; }
    if (!code) { fail("CreateShaderModule: null shader text"); return nullptr; }
    const std::string text(code, size);
    // The reference JIT-compiles `code` and takes the kernel named "raygen" (radiance.cpp:152-179).  Three cases here:
    //  1. the text IS the reference's stock program (samples/shader.cl, recognised by a hash of its non-blank characters): its
    //     stage functions are the ones of samples/sbt.json that this library ships as hand-written HIP -> wavefront pipeline;
    //  2. `raygen` declared without parameters: a placeholder that asks for the stock pipeline (nothing could be bound to it);
    //  3. any other program: compiled at run time by ROCm's OpenCL C compiler and run as the megakernel it is (user_shader.cpp).
    const std::string bare = strip_comments(text);
    if (!has_identifier(bare, "raygen")) {
        fail("CreateShaderModule: shader text has no `raygen` kernel (clCreateKernel(\"raygen\") would fail)");
        return nullptr;
    }
    auto s = std::make_unique<rdx_shader_s>();
    s->name = name ? name : "";
    s->hasRaygen = true;
    constexpr uint64_t kStockShaderHash = 0xc0cc932e07087140ull;      // FNV-1a-64 of samples/shader.cl without white space (16 983 characters)
    const bool stock = fnv1a64_nows(text) == kStockShaderHash || raygen_has_parameters(bare) == 0;
    if (!stock) {
        if (g_ndev > 1) { fail("CreateShaderModule: user shader programs are not supported in multi-device mode"); return nullptr; }
        hipDeviceProp_t prop;
        HIP_OKP(hipGetDeviceProperties(&prop, g0.device));
        std::string arch = prop.gcnArchName;
        arch = arch.substr(0, arch.find(':'));
        std::string err;
        // 3a. the program differs from the stock one only INSIDE its closest-hit / miss stage functions (blank_stage_bodies):
        //     those functions are compiled into the shade stage of the wavefront pipeline (user_shader.cpp "stage mode");
        // 3b. anything else: the program's own raygen, as a megakernel.
        constexpr uint64_t kStockReducedHash = RDX_STOCK_REDUCED_HASH;     // of samples/shader.cl, by tools/stock_shader_hash.py
        //     "user_stages" 2: the caller asserts it for a program written from scratch (the raygen text is then not looked at).
        const bool stages = g0.opt.userStages == 2 || (g0.opt.userStages == 1 && stage_reduced_hash(text) == kStockReducedHash);
        if (stages) {
            // the stage kernel replaces the program's raygen: its body and that of the stock skeleton's camera helper go (dead
            // code there, and their get_global_id(0) has no `sceneData` in scope for the stage-mode macro)
            std::string t = bare;
            blank_bodies(t, {"raygen", "generateRay"});
            std::string err2;
            s->program = compile_user_shader(t, g0.shaderInclude, arch, true, err2);
            if (!s->program && g0.opt.userStages == 2) { fail_str(err2); return nullptr; }
        }
        if (!s->program) s->program = compile_user_shader(text, g0.shaderInclude, arch, false, err);
        if (!s->program) { fail_str(err); return nullptr; }
    }
    g.shaders.push_back(std::move(s));
    return g.shaders.back().get();
}

extern "C" int rdx_bind_pipeline(rdx_shader m)
{
    if (!m) return fail("BindPipeline: null shader module");
    g.pipeline = m;
    return 0;
}

extern "C" int rdx_bind_descriptor_set(void* const* handles, uint32_t n)
{
    if (!g.pipeline) return fail("BindDescriptorSet: no pipeline bound");
    if (n > 14) return fail("BindDescriptorSet: %u descriptors, the raygen stage takes 14", n);
    for (uint32_t i = 0; i < n; ++i) g.slots[i] = handles[i];
    g.nslots = std::max(g.nslots, n);
    return 0;
}

// ------------------------------------------------------------------------------------------------
// sharding
// ------------------------------------------------------------------------------------------------
extern "C" int rdx_set_shard(uint32_t rank, uint32_t world, uint32_t tw, uint32_t th)
{
    if (world == 0 || rank >= world || tw == 0 || th == 0) return fail("rdx_set_shard: invalid rank/world/tile");
    g.rank = rank; g.world = world; g.tileW = tw; g.tileH = th;
    return 0;
}

extern "C" uint32_t rdx_shard_pixel_count(uint32_t w, uint32_t h, uint32_t rank, uint32_t world)
{
    std::vector<uint32_t> px;
    owned_pixel_list(w, h, g.tileW, g.tileH, rank, world, px);
    return (uint32_t)px.size();
}

static int pack_impl(rdx_buffer image, rdx_buffer packed, uint32_t w, uint32_t h, uint32_t elem, uint32_t rank,
                     uint32_t world, bool unpack)
{
    if (!image || !packed || !known_buffer(image) || !known_buffer(packed)) return fail("pack_tiles: invalid buffer");
    if (elem % 4 || elem == 0) return fail("pack_tiles: element size must be a multiple of 4");
    const uint32_t tilesX = (w + g.tileW - 1) / g.tileW, tilesY = (h + g.tileH - 1) / g.tileH, nT = tilesX * tilesY;
    const uint32_t owned = nT > rank ? (nT - rank + world - 1) / world : 0;
    if ((size_t)w * h * elem > image->size) return fail("pack_tiles: image buffer too small");
    if ((size_t)owned * g.tileW * g.tileH * elem > packed->size) return fail("pack_tiles: packed buffer too small");
    launch_pack_tiles(g.stream, static_cast<uint8_t*>(dp(image)), static_cast<uint8_t*>(dp(packed)), w, h, elem,
                      g.tileW, g.tileH, rank, world, unpack);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    if (unpack) image->version++; else packed->version++;
    return 0;
}
extern "C" int rdx_pack_tiles(rdx_buffer image, rdx_buffer packed, uint32_t w, uint32_t h, uint32_t elem, uint32_t rank, uint32_t world)
{ return pack_impl(image, packed, w, h, elem, rank, world, false); }
extern "C" int rdx_unpack_tiles(rdx_buffer packed, rdx_buffer image, uint32_t w, uint32_t h, uint32_t elem, uint32_t rank, uint32_t world)
{ return pack_impl(image, packed, w, h, elem, rank, world, true); }
// the gathering rank's side of a frame: the packed buffers of ranks first_rank .. first_rank + n - 1 go into the image with
// ONE synchronisation at the end (a call per rank costs a launch + a stream synchronise each: 7 of them per frame at 8 GPUs)
extern "C" int rdx_unpack_tiles_multi(const rdx_buffer* packed, uint32_t first_rank, uint32_t n, rdx_buffer image, uint32_t w, uint32_t h,
                                      uint32_t elem, uint32_t world)
{
    if (!packed || !image || !known_buffer(image)) return fail("unpack_tiles_multi: invalid buffer");
    if (elem % 4 || elem == 0) return fail("unpack_tiles_multi: element size must be a multiple of 4");
    if ((size_t)w * h * elem > image->size) return fail("unpack_tiles_multi: image buffer too small");
    const uint32_t tilesX = (w + g.tileW - 1) / g.tileW, tilesY = (h + g.tileH - 1) / g.tileH, nT = tilesX * tilesY;
    for (uint32_t k = 0; k < n; ++k) {          // validate everything before anything is launched
        const uint32_t rank = first_rank + k;
        if (rank >= world || !packed[k] || !known_buffer(packed[k])) return fail("unpack_tiles_multi: invalid packed buffer %u", k);
        const uint32_t owned = nT > rank ? (nT - rank + world - 1) / world : 0;
        if ((size_t)owned * g.tileW * g.tileH * elem > packed[k]->size) return fail("unpack_tiles_multi: packed buffer %u too small", k);
    }
    for (uint32_t k = 0; k < n; ++k) {
        const uint32_t rank = first_rank + k;
        launch_pack_tiles(g.stream, static_cast<uint8_t*>(image->dptr), static_cast<uint8_t*>(packed[k]->dptr), w, h, elem,
                          g.tileW, g.tileH, rank, world, true);
    }
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    image->version++;
    return 0;
}

// ------------------------------------------------------------------------------------------------
// TraceRays
// ------------------------------------------------------------------------------------------------
extern "C" int rdx_set_profiling(int on) { g.opt.profiling = on != 0; return 0; }
extern "C" int rdx_set_option(const char* name, int64_t value)
{
    if (!name) return fail("rdx_set_option: null name");
    if (!strcmp(name, "chunk_paths")) { if (value < 1) return fail("chunk_paths must be >= 1"); g.opt.chunkPaths = value; return 0; }
    if (!strcmp(name, "count_visits")) { g.opt.countVisits = value != 0; return 0; }
    if (!strcmp(name, "groups")) { if (value < 0 || value > Context::MAX_GROUPS) return fail("groups must be 0 (auto) or 1..4"); g.opt.groupsOpt = (int)value; return 0; }
    if (!strcmp(name, "overlap")) { if (value < 0 || value > 1) return fail("overlap must be 0 or 1"); g.opt.overlap = (int)value; return 0; }
    if (!strcmp(name, "pipeline")) { if (value < 0 || value > 1) return fail("pipeline must be 0 (staged) or 1 (paths)"); g.opt.pathMode = (int)value; return 0; }
    if (!strcmp(name, "fuse")) { if (value < -1 || value > 1) return fail("fuse must be -1 (auto), 0 or 1"); g.opt.fuse = (int)value; return 0; }
    if (!strcmp(name, "user_shader_local_size")) { if (value < 1 || value > 1024) return fail("user_shader_local_size must be 1..1024"); g.opt.userLocalSize = (int)value; return 0; }
    if (!strcmp(name, "sort")) { g.opt.sortRays = value < 0 ? -1 : (value != 0); return 0; }
    if (!strcmp(name, "textures")) { g.opt.textures = value != 0; return 0; }
    if (!strcmp(name, "cull")) { g.opt.cull = value < 0 ? -1 : (value != 0); return 0; }
    if (!strcmp(name, "top_flat")) { g.opt.topFlat = value != 0; return 0; }
    if (!strcmp(name, "group_instances")) { g.opt.groupInstances = value != 0; return 0; }
    if (!strcmp(name, "group_entry_items")) { g.opt.groupEntryItems = value != 0; return 0; }
    if (!strcmp(name, "unified_tree")) { g.opt.unifiedTree = value != 0; return 0; }
    if (!strcmp(name, "gpu_build") || !strcmp(name, "gpu_build_min")) {
        if (!strcmp(name, "gpu_build")) g0.gpuBuild = value != 0; else g0.gpuBuildMin = value > 0 ? value : 32768;
        set_gpu_binner((g0.initialized && g0.gpuBuild) ? &g_hipBinner : nullptr, (size_t)g0.gpuBuildMin);
        return 0;
    }
    if (!strcmp(name, "sort_min_paths")) { g.opt.sortMinPaths = value > 0 ? value : (3ll << 19); return 0; }
    if (!strcmp(name, "small_chunk_paths")) { g.opt.smallChunkPaths = value > 0 ? value : (9ll << 19); return 0; }
    if (!strcmp(name, "quad")) { g.opt.quad = value < 0 ? -1 : (value != 0); return 0; }
    if (!strcmp(name, "user_stages")) { g.opt.userStages = value > 2 ? 1 : (int)value; return 0; }
    if (!strcmp(name, "inline_leaf_roots")) { g.opt.inlineLeafRoots = value != 0; return 0; }
    if (!strcmp(name, "kernel")) { if (value < 0 || value > 3) return fail("kernel must be 0, 1, 2 or 3"); g.opt.kernel = (int)value; return 0; }
    return fail("rdx_set_option: unknown option '%s'", name);
}
extern "C" int rdx_get_bounce_counts(uint64_t* out, uint32_t n)
{
    if (!out) return fail("null");
    for (uint32_t d = 0; d < n && d < 65; ++d) out[d] = g.bounceCounts[d];
    return 0;
}

extern "C" int rdx_get_visit_profile(uint64_t* out, uint32_t max_bounces)
{
    if (!out) return fail("null");
    const uint32_t n = std::min(max_bounces, g.visitDepth);
    for (uint32_t d = 0; d < n; ++d)
        for (int k = 0; k < 8; ++k) out[8 * d + k] = g.hVisit[8 * d + k];
    return (int)n;
}

extern "C" int rdx_get_trace_stats(rdx_trace_stats* out) { if (!out) return fail("null"); *out = g.stats; return 0; }

// ---- the bounces of a chunk: what rdx_trace_rays and rdx_trace_paths share ----------------------------------------------------
// The engine's view, the scene and the switches of one chunk.  nPixels / sampleBase place a finished path's colour in
// PathStreams::sampleColor (kernels.hip store_sample: [(frameID - sampleBase) * nPixels + slot]); with 0 / 0 it is record `slot`.
struct BounceArgs {
    rdx_buffer_s* tlas; AccelView av; SceneArgs sc;
    uint32_t maxDepth, nPixels, sampleBase;
    bool fuse, overlap, sortOn; SortBox sortBox;
    unsigned long long* visit;
    float tmin, tmax;
};

// fuse / overlap / sortOn / sortBox of a chunk of `chunkPaths` paths from the options, B.av, B.visit and the scene of B.tlas
static void bounce_switches(uint64_t chunkPaths, BounceArgs& B)
{
    const auto& S = acc(B.tlas)->s;
    // Small chunks (multi-GPU shards, low resolutions): a traversal launch costs ~0.2 ms of ramp + tail
    // whatever its size (tools/trav_scale.py), so shadow(d) and extend(d+1) -- same ray count, disjoint
    // streams -- go into ONE cooperative launch: 9 traversal launches per depth-8 frame instead of 16.
    B.fuse = g.opt.fuse != 0 && !B.visit && B.av.kernel >= 2;
    B.overlap = g.opt.overlap == 1 && !B.fuse && !B.visit;
    // per-bounce ray sort (north star; kernels.h): only the cooperative engines hand rays out by index
    B.sortOn = !B.visit && B.av.kernel >= 2 &&
               (g.opt.sortRays > 0 || (g.opt.sortRays < 0 && (S.nWide >= RDX_SORT_AUTO_MIN_WIDE ||
                                                              (S.nWide >= RDX_SORT_AUTO_MIN_WIDE_FULL && chunkPaths > (uint64_t)g.opt.sortMinPaths))));
    for (int k = 0; k < 3; ++k) {
        const float lo = S.sceneLo[k], ext = S.sceneHi[k] - lo;
        B.sortBox.lo[k] = lo; B.sortBox.inv[k] = ext > 0.0f ? 16.0f / ext : 0.0f;
    }
}

// the sort scratch of a group, allocated on first use: the two copies of total[] start as zeros (stream-ordered before the group's
// first sort); from then on every sort leaves the copy its successor counts into zeroed (kernels.h)
static int ensure_sort_bins(Context::Group& G)
{
    if (G.sortBins) return 0;
    HIP_OK(hipMalloc(reinterpret_cast<void**>(&G.sortBins), (size_t)ray_sort_tiles_words() * 4));
    HIP_OK(hipMemsetAsync(G.sortBins, 0, (size_t)ray_sort_zeroed_words() * 4, G.s0));
    G.sortPhase = 0;
    return 0;
}

// gps[k]: the streams of group k, its gPaths[k] paths generated and their first hits found (G.dCounts[0] = gPaths[k], device side).
// Nothing is synchronised; on return gps[k] holds the streams as the last bounce left them.
static int trace_bounces(const BounceArgs& B, PathStreams* gps, const uint32_t* gPaths, int nGroups)
{
    // Per bounce and group:  shade(d) -> { shadow(d), extend(d+1) } -> shade(d+1) ...
    // shadow(d) only fills nCol (or the final sample colour) and reads streams nobody writes meanwhile;
    // extend(d+1) reads the next-bounce rays shade(d) wrote.  The two are traced by one fused launch,
    // by two launches back to back, or (overlap) on two streams.
    for (uint32_t d = 0; d < B.maxDepth; ++d) {
        for (int k = 0; k < nGroups; ++k) {
            Context::Group& G = g.groups[k];
            PathStreams& ps = gps[k];
            const uint32_t n0 = gPaths[k];
            const bool last = d + 1 == B.maxDepth;
            if (B.overlap && d > 0) HIP_OK(hipStreamWaitEvent(G.s0, G.evShadow[d - 1], 0));   // shade(d) reads col written by shadow(d-1)
            g_timer.begin(&g.stats.ms_shade, G.s0);
            if (B.sortOn && G.permCap < n0) {
                if (G.permE) HIP_IGN(hipFree(G.permE));
                if (G.sortKey) HIP_IGN(hipFree(G.sortKey));
                G.permE = nullptr; G.sortKey = nullptr; G.permCap = 0;
                HIP_OK(hipMalloc(reinterpret_cast<void**>(&G.permE), (size_t)n0 * 4));
                HIP_OK(hipMalloc(reinterpret_cast<void**>(&G.sortKey), (size_t)n0 * 2));
                G.permCap = n0;
            }
            ps.sortKey = B.sortOn ? G.sortKey : nullptr;        // (the shade stage writes the survivors' sort keys)
            launch_shade(G.s0, B.av, B.sc, ps, G.dCounts + d, G.dCounts + d + 1, n0, d, B.maxDepth, B.nPixels, B.sampleBase, B.sortOn ? &B.sortBox : nullptr);
            g_timer.end(G.s0);
            ps.permS = nullptr; ps.permE = nullptr;
            if (B.sortOn) {
                // per-bounce ray sort: the traversal launch below hands its rays out in (octant, Morton cell) order
                if (ensure_sort_bins(G)) return -1;
                g_timer.begin(&g.stats.ms_sort, G.s0);
                launch_ray_sort_tiles(G.s0, ps, G.dCounts + d + 1, n0, B.sortBox, G.sortBins, G.sortPhase, G.permE,
                                      ray_sort_key_bits(acc(B.tlas)->s.nWide >= RDX_SORT_AUTO_MIN_WIDE));
                g_timer.end(G.s0);
                ps.permS = G.permE; ps.permE = G.permE;
            }
            const PathStreams psShadow = ps;
            // the compacted survivors become the live paths of the next bounce
            std::swap(ps.rayO, ps.nRayO); std::swap(ps.rayD, ps.nRayD); std::swap(ps.thr, ps.nThr); std::swap(ps.col, ps.nCol);
            if (B.fuse && !last) {
                g_timer.begin(&g.stats.ms_fused, G.s0);
                launch_fused(G.s0, B.av, B.sc, psShadow, ps, G.dCounts + d + 1, n0, B.nPixels, B.sampleBase, B.tmin, B.tmax, G.dCounts + 128 + d);
                g_timer.end(G.s0);
                g.stats.launches_shadow++; g.stats.launches_extend++;
                continue;
            }
            hipStream_t ss = G.s0;
            if (B.overlap) {
                HIP_OK(hipEventRecord(G.evShade[d], G.s0));
                HIP_OK(hipStreamWaitEvent(G.s1, G.evShade[d], 0));
                ss = G.s1;
            }
            g_timer.begin(&g.stats.ms_shadow, ss);
            launch_shadow(ss, B.av, B.sc, psShadow, G.dCounts + d + 1, n0, last, B.nPixels, B.sampleBase, B.tmin, B.tmax, B.visit ? B.visit + 8 * d : nullptr,
                          G.dCounts + 128 + d);
            g_timer.end(ss);
            if (B.overlap) HIP_OK(hipEventRecord(G.evShadow[d], G.s1));
            g.stats.launches_shadow++;
            if (!last) {
                g_timer.begin(&g.stats.ms_extend, G.s0);
                launch_extend(G.s0, B.av, ps, G.dCounts + d + 1, n0, B.tmin, B.tmax, B.visit ? B.visit + 8 * (d + 1) : nullptr, G.dCounts + 64 + d + 1);
                g_timer.end(G.s0);
                g.stats.launches_extend++;
            }
        }
    }
    return 0;
}

// the groups' live counts of a finished chunk (hCounts, read back) into the ray counts of the call
static void add_group_counts(int nGroups, uint32_t maxDepth)
{
    for (int k = 0; k < nGroups; ++k) {
        const uint32_t* hc = g.groups[k].hCounts;
        for (uint32_t d = 0; d <= maxDepth && maxDepth; ++d) g.bounceCounts[d] += hc[d];
        if (maxDepth) g.stats.rays_primary += hc[0];
        for (uint32_t d = 1; d < maxDepth; ++d) g.stats.rays_bounce += hc[d];
        for (uint32_t d = 0; d < maxDepth; ++d) { g.stats.rays_shadow += hc[d + 1]; g.stats.closest_hits += hc[d + 1]; }
    }
}

// one frame on the calling thread's device (context `g`, logical device tl_dev): every pixel of its shard
static int trace_rays_device(uint32_t width, uint32_t height)
{
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!g.pipeline) return fail("TraceRays: no pipeline bound");
    if (g.nslots < 14) return fail("TraceRays: %u descriptors bound, the raygen stage takes 14", g.nslots);
    for (int i : {0, 1, 2, 3, 13})
        if (!g.slots[i] || !known_buffer(g.slots[i])) return fail("descriptor slot %d is not a buffer", i);
    auto* bRT = static_cast<rdx_buffer_s*>(g.slots[0]);
    auto* bScratch = static_cast<rdx_buffer_s*>(g.slots[1]);
    auto* bImage = static_cast<rdx_buffer_s*>(g.slots[2]);
    auto* bCam = static_cast<rdx_buffer_s*>(g.slots[3]);
    auto* bTlas = static_cast<rdx_buffer_s*>(g.slots[13]);
    const uint64_t nPix = (uint64_t)width * height;
    if (nPix == 0) return 0;
    if (g.pipeline->program && !g.pipeline->program->stages) {
        // a user's own raygen program: the megakernel, one work-item per pixel, bound by position like clSetKernelArg
        // (radiance.cpp:231-259); slots 11 / 12 (texture array, sampler) are passed as the library's views of them (user_tex_views)
        if (nPix > 0xffffffffull) return fail("TraceRays: too many pixels");
        void* ptrs[14];
        const int slotOf[12] = {0, 1, 2, 3, 4, 5, 6, 7, 8, 9, 10, 13};
        for (int i = 0; i < 12; ++i) {
            void* h = g.slots[slotOf[i]];
            if (!h || !known_buffer(h)) return fail("descriptor slot %d is not a buffer", slotOf[i]);
            ptrs[i] = dp(static_cast<rdx_buffer_s*>(h));
        }
        if (user_tex_views(ptrs[12], ptrs[13])) return -1;
        std::memset(&g.stats, 0, sizeof g.stats);
        g.stats.pixels = nPix;
        HIP_OK(hipEventRecord(g.evA, g.stream));
        std::string err;
        if (launch_user_shader(g.pipeline->program, g.stream, ptrs, (uint32_t)nPix, (uint32_t)g.opt.userLocalSize, err)) return fail_str(err);
        HIP_OK(hipEventRecord(g.evB, g.stream));
        HIP_OK(hipStreamSynchronize(g.stream));
        HIP_OK(hipEventElapsedTime(&g.stats.ms_total, g.evA, g.evB));
        // the program wrote imageScratch / image itself: host mirrors of nothing are affected (only RTProp / camera are mirrored,
        // and a raygen that wrote them would be outside the reference's host contract, sample1.cpp:480-490)
        return 0;
    }
    if (nPix > 0x7fffffffull) return fail("TraceRays: %llu pixels exceed the 31-bit pixel index", (unsigned long long)nPix);
    if (bRT->size < sizeof(RayTraceProperties) || bCam->size < sizeof(PhysicalCamera)) return fail("TraceRays: RTProp / camera buffer too small");
    if (bScratch->size < nPix * 16) return fail("TraceRays: imageScratch holds %zu bytes, %llu needed", bScratch->size, (unsigned long long)nPix * 16);
    if (bImage->size < nPix * 4) return fail("TraceRays: image holds %zu bytes, %llu needed", bImage->size, (unsigned long long)nPix * 4);

    SceneArgs sc;
    if (scene_args(sc)) return -1;
    if (derive_accel(bTlas)) return -1;

    // per-frame constants live in device buffers the caller may have rewritten (sample1.cpp:480-490)
    RayTraceProperties rt; PhysicalCamera cam;
    if (bRT->mirrorValid && bRT->mirror.size() >= sizeof rt) std::memcpy(&rt, bRT->mirror.data(), sizeof rt);
    else HIP_OK(hipMemcpy(&rt, dp(bRT), sizeof rt, hipMemcpyDeviceToHost));
    if (bCam->mirrorValid && bCam->mirror.size() >= sizeof cam) std::memcpy(&cam, bCam->mirror.data(), sizeof cam);
    else HIP_OK(hipMemcpy(&cam, dp(bCam), sizeof cam, hipMemcpyDeviceToHost));
    CameraArgs C;
    if (camera_args(cam, C)) return -1;
    if ((uint32_t)cam.widthPixel == 0) return fail("TraceRays: camera widthPixel is 0");

    if (ensure_owned(width, height)) return -1;
    const uint32_t P = g.ownedCount;
    const uint32_t* owned = g.world > 1 ? g.ownedPixels : nullptr;

    // depth as the raygen loop sees it: `debug` breaks after the first bounce (shader.cl:256-259)
    uint32_t maxDepth = rt.depth;
    if (rt.debug && maxDepth > 1) maxDepth = 1;
    if (maxDepth > 62) return fail("TraceRays: depth %u exceeds the supported maximum of 62", maxDepth);

    std::memset(&g.stats, 0, sizeof g.stats);
    std::memset(g.bounceCounts, 0, sizeof g.bounceCounts);
    g.stats.pixels = P;
    unsigned long long* visit = g.opt.countVisits ? g.dVisit : nullptr;
    if (visit) HIP_OK(hipMemsetAsync(g.dVisit, 0, 64 * 8 * sizeof(unsigned long long), g.stream));

    HIP_OK(hipEventRecord(g.evA, g.stream));
    const uint32_t batch = rt.batchSize;
    uint32_t samplesPerChunk = batch;
    if (P && (uint64_t)batch * P > (uint64_t)g.opt.chunkPaths) samplesPerChunk = (uint32_t)std::max<int64_t>(1, g.opt.chunkPaths / P);
    if (P && batch) { if (ensure_samples((size_t)samplesPerChunk * P)) return -1; }
    // quad records (two tree levels per fetch, kernels at 4 waves per SIMD) for chunks whose launches do not fill the chip --
    // shards of a multi-GPU frame, low resolutions -- where a launch lasts as long as its longest chain of dependent fetches
    const AccelView av = view_of(bTlas, (uint64_t)samplesPerChunk * P <= (uint64_t)g.opt.sortMinPaths);

    const float tmin = 0.001f, tmax = 1000.0f;      // shader.cl:235-236, 500
    for (uint32_t s0 = 0; s0 < batch && P; s0 += samplesPerChunk) {
        const uint32_t sc_n = std::min(samplesPerChunk, batch - s0);
        const uint32_t sampleBase = rt.totalSamples + s0;
        const uint64_t chunkPaths = (uint64_t)sc_n * P;
        // Small chunks (multi-GPU shards, low resolutions): a persistent traversal launch costs ~0.19 ms of ramp +
        // drain whatever its size (profiles/r01k_timeline_eighth_before_groups.txt: 9 launches = 1.7 of the 3.7 ms of a 1/8 frame).
        // The chunk's samples are split into groups with their own streams and counts, each launching 1/nGroups of
        // the resident grid, so that one group's launches run inside the ramp and drain of the other's
        // (kernels.hip: set_grid_share).  Two groups: -5 % at 1/8, -3 % at 1/2 of a 1080p x 4 spp frame; four: slower.
        const bool small = chunkPaths <= (uint64_t)g.opt.smallChunkPaths && sc_n >= 2 && av.kernel >= 2;
        const uint32_t wantGroups = visit ? 1u : g.opt.groupsOpt ? (uint32_t)g.opt.groupsOpt : small ? 2u : 1u;
        int nGroups = (int)std::min<uint32_t>(wantGroups, sc_n);
        set_grid_share((uint32_t)nGroups);
        g.stats.groups = (uint32_t)nGroups;
        BounceArgs B{bTlas, av, sc, maxDepth, P, sampleBase, false, false, false, SortBox{}, visit, tmin, tmax};
        bounce_switches(chunkPaths, B);
        HIP_OK(hipEventRecord(g.evChunk, g.stream));          // everything before this chunk (previous accumulate) is done first

        if (g.pipeline->program && g.pipeline->program->stages) {
            // ---- a user's stage functions on the wavefront pipeline (user_shader.cpp "stage mode") --------------------------------
            // generate -> extend(0) -> [ stage pass 0 (records the shader's shadow query) -> shadow walk -> stage pass 1 (the shader
            // again, the query answered; raygen bookkeeping; compaction) -> extend(d + 1) ] ... -> accumulate.  One group, no fusing:
            // extend(d + 1) needs pass 1's rays.
            if (av.kernel != 3) return fail("TraceRays: user stage functions need the pool engine (kernel 3)");
            Context::Group& G = g.groups[0];
            const uint32_t n0 = sc_n * P;
            if (ensure_group(G, n0)) return -1;
            if (G.stageCap < n0) {
                float4** arr[] = {&G.ps.shD, &G.ps.payC, &G.ps.payF, &G.ps.nPayC, &G.ps.nPayF};
                for (auto a : arr) { if (*a) HIP_IGN(hipFree(*a)); *a = nullptr; HIP_OK(hipMalloc(reinterpret_cast<void**>(a), (size_t)n0 * sizeof(float4))); }
                if (G.ps.shHit) HIP_IGN(hipFree(G.ps.shHit));
                G.ps.shHit = nullptr;
                HIP_OK(hipMalloc(reinterpret_cast<void**>(&G.ps.shHit), (size_t)n0 * sizeof(uint32_t)));
                G.stageCap = n0;
            }
            G.ps.sampleColor = g.sampleColor;
            PathStreams ps = G.ps;
            std::memset(G.hCounts, 0, 256 * sizeof(uint32_t));
            G.hCounts[0] = n0;
            HIP_OK(hipMemcpyAsync(G.dCounts, G.hCounts, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
            launch_generate(g.stream, C, ps, owned, P, s0, sc_n, rt.totalSamples);
            if (maxDepth == 0) launch_finalize_all(g.stream, ps, n0, P, sampleBase);
            else launch_extend(g.stream, av, ps, G.dCounts, n0, tmin, tmax, nullptr, G.dCounts + 64);
            void* slotPtr[14];
            for (int i = 0; i < 14; ++i) slotPtr[i] = (g.slots[i] && known_buffer(g.slots[i])) ? dp(static_cast<rdx_buffer_s*>(g.slots[i])) : nullptr;
            void *texImage = nullptr, *texSampler = nullptr;
            if (user_tex_views(texImage, texSampler)) return -1;
            for (uint32_t d = 0; d < maxDepth; ++d) {
                for (uint32_t pass = 0; pass < 2; ++pass) {
                    const uint32_t scalars[6] = {pass, d, maxDepth, P, sampleBase, rt.debug};
                    void* ptrs[33] = {G.dCounts + d, G.dCounts + d + 1, G.dCounts + 200,
                                      slotPtr[3], slotPtr[4], slotPtr[5], slotPtr[6], slotPtr[7], slotPtr[8], slotPtr[9], slotPtr[10], slotPtr[13],
                                      const_cast<DInst*>(av.insts),
                                      ps.rayO, ps.rayD, ps.thr, ps.col, ps.hitA, ps.hitInst, ps.payC, ps.payF,
                                      ps.shO, ps.shD, ps.shHit,
                                      ps.nRayO, ps.nRayD, ps.nThr, ps.nCol, ps.nPayC, ps.nPayF, ps.sampleColor, texImage, texSampler};
                    std::string err;
                    if (launch_user_stage(g.pipeline->program, g.stream, scalars, ptrs, n0, err)) return fail_str(err);
                    if (pass == 0) launch_shadow_user(g.stream, av, ps, G.dCounts + d, n0, tmin, tmax, G.dCounts + 128 + d);
                }
                std::swap(ps.rayO, ps.nRayO); std::swap(ps.rayD, ps.nRayD); std::swap(ps.thr, ps.nThr); std::swap(ps.col, ps.nCol);
                std::swap(ps.payC, ps.nPayC); std::swap(ps.payF, ps.nPayF);
                if (d + 1 < maxDepth) launch_extend(g.stream, av, ps, G.dCounts + d + 1, n0, tmin, tmax, nullptr, G.dCounts + 64 + d + 1);
            }
            launch_accumulate(g.stream, ps, owned, P, s0, sc_n, rt.totalSamples, s0 + sc_n >= batch, rt.debug,
                              static_cast<float*>(dp(bScratch)), static_cast<uint8_t*>(dp(bImage)));
            HIP_OK(hipMemcpyAsync(G.hCounts, G.dCounts, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
            HIP_OK(hipStreamSynchronize(g.stream));
            if (G.hCounts[200] != 0)
                return fail("TraceRays: the program's closest-hit shader cannot run on the wavefront pipeline (%s); rdx_set_option(\"user_stages\", 0) runs it as a megakernel",
                            (G.hCounts[200] & 4u) ? "it calls traceRay more than once" : "its nested traceRay is not the stock shadow query: sbtRecordOffset 2, Tmin 0.001, Tmax 1000");
            const uint32_t* hc = G.hCounts;
            if (maxDepth) g.stats.rays_primary += hc[0];
            for (uint32_t d = 1; d < maxDepth; ++d) g.stats.rays_bounce += hc[d];
            for (uint32_t d = 0; d <= maxDepth && maxDepth; ++d) g.bounceCounts[d] += hc[d];
            g.stats.launches_extend += maxDepth; g.stats.launches_shadow += maxDepth;
            continue;
        }
        if (g.opt.pathMode == 1 && !visit && av.kernel == 3 && maxDepth > 0) {
            // ---- whole paths in one persistent launch (k_path_pool) + accumulate ----
            Context::Group& G = g.groups[0];
            const uint32_t n0 = sc_n * P;
            if (ensure_group(G, n0)) return -1;
            G.ps.sampleColor = g.sampleColor;
            std::memset(G.hCounts, 0, 256 * sizeof(uint32_t));
            HIP_OK(hipMemcpyAsync(G.dCounts, G.hCounts, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, g.stream));
            unsigned long long* tally = reinterpret_cast<unsigned long long*>(G.dCounts + 192);     // 8-byte aligned words 192..195
            g_timer.begin(&g.stats.ms_path);
            launch_path(g.stream, av, sc, C, G.ps, owned, P, s0, sc_n, rt.totalSamples, maxDepth, sampleBase, G.dCounts + 64, tally, tmin, tmax);
            g_timer.end();
            g_timer.begin(&g.stats.ms_accumulate);
            launch_accumulate(g.stream, G.ps, owned, P, s0, sc_n, rt.totalSamples, s0 + sc_n >= batch, rt.debug,
                              static_cast<float*>(dp(bScratch)), static_cast<uint8_t*>(dp(bImage)));
            g_timer.end();
            HIP_OK(hipMemcpyAsync(G.hCounts, G.dCounts, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, g.stream));
            HIP_OK(hipStreamSynchronize(g.stream));
            const unsigned long long* ht = reinterpret_cast<const unsigned long long*>(G.hCounts + 192);
            g.stats.rays_primary += n0;
            g.stats.rays_bounce += ht[0] - n0;
            g.stats.rays_shadow += ht[1];
            g.stats.closest_hits += ht[1];
            g.stats.launches_extend++;
            continue;
        }

        uint32_t gBegin[Context::MAX_GROUPS + 1];
        for (int k = 0; k <= nGroups; ++k) gBegin[k] = (uint32_t)((uint64_t)sc_n * k / nGroups);
        PathStreams gps[Context::MAX_GROUPS];
        uint32_t gPaths[Context::MAX_GROUPS];
        for (int k = 0; k < nGroups; ++k) {
            Context::Group& G = g.groups[k];
            const uint32_t ns = gBegin[k + 1] - gBegin[k], n0 = ns * P;
            gPaths[k] = n0;
            if (ensure_group(G, n0)) return -1;
            G.ps.sampleColor = g.sampleColor;
            gps[k] = G.ps;
            if (k > 0) HIP_OK(hipStreamWaitEvent(G.s0, g.evChunk, 0));
            std::memset(G.hCounts, 0, 256 * sizeof(uint32_t));
            G.hCounts[0] = n0;
            HIP_OK(hipMemcpyAsync(G.dCounts, G.hCounts, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, G.s0));
            g_timer.begin(&g.stats.ms_generate, G.s0);
            launch_generate(G.s0, C, gps[k], owned, P, s0 + gBegin[k], ns, rt.totalSamples);
            g_timer.end(G.s0);
            if (maxDepth == 0) launch_finalize_all(G.s0, gps[k], n0, P, sampleBase);
            if (maxDepth > 0) {
                g_timer.begin(&g.stats.ms_extend, G.s0);
                launch_extend(G.s0, av, gps[k], G.dCounts, n0, tmin, tmax, visit, G.dCounts + 64);     // visit row 0
                g_timer.end(G.s0);
                g.stats.launches_extend++;
            }
        }
        if (trace_bounces(B, gps, gPaths, nGroups)) return -1;
        for (int k = 0; k < nGroups; ++k) {
            Context::Group& G = g.groups[k];
            if (B.overlap && maxDepth > 0) HIP_OK(hipStreamWaitEvent(G.s0, G.evShadow[maxDepth - 1], 0));
            HIP_OK(hipMemcpyAsync(G.hCounts, G.dCounts, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, G.s0));
            if (k > 0) { HIP_OK(hipEventRecord(G.evDone, G.s0)); HIP_OK(hipStreamWaitEvent(g.stream, G.evDone, 0)); }
        }
        g_timer.begin(&g.stats.ms_accumulate);
        launch_accumulate(g.stream, gps[0], owned, P, s0, sc_n, rt.totalSamples, s0 + sc_n >= batch, rt.debug,
                          static_cast<float*>(dp(bScratch)), static_cast<uint8_t*>(dp(bImage)));
        g_timer.end();
        HIP_OK(hipStreamSynchronize(g.stream));
        add_group_counts(nGroups, maxDepth);
    }
    if (batch == 0 && P) {
        // no samples: only the tonemap of the existing accumulator runs (shader.cl:283-304)
        PathStreams none{};
        launch_accumulate(g.stream, none, owned, P, 0, 0, rt.totalSamples, true, rt.debug,
                          static_cast<float*>(dp(bScratch)), static_cast<uint8_t*>(dp(bImage)));
    }
    HIP_OK(hipEventRecord(g.evB, g.stream));
    if (visit) HIP_OK(hipMemcpyAsync(g.hVisit, g.dVisit, 64 * 8 * sizeof(unsigned long long), hipMemcpyDeviceToHost, g.stream));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));          // clFinish (radiance.cpp:261)
    if (take_status()) return fail("TraceRays: a traversal wave exceeded its iteration bound and gave up (internal error in the step selection); the frame is incomplete");
    HIP_OK(hipEventElapsedTime(&g.stats.ms_total, g.evA, g.evB));
    g_timer.resolve();
    g.visitDepth = 0;
    if (visit) {
        g.visitDepth = maxDepth;
        for (uint32_t d = 0; d < maxDepth; ++d)
            for (int c = 0; c < 2; ++c) {
                const unsigned long long* v = g.hVisit + 8 * d + 4 * c;
                g.stats.visit_top_nodes[c] += v[0]; g.stats.visit_instances[c] += v[1];
                g.stats.visit_bot_nodes[c] += v[2]; g.stats.visit_triangles[c] += v[3];
            }
    }
    bScratch->version++; bImage->version++;
    return 0;
}

static int ensure_stage(int slot, size_t bytes)
{
    if (g.gatherCap[slot] >= bytes) return 0;
    if (g.gatherStage[slot]) HIP_IGN(hipFree(g.gatherStage[slot]));
    g.gatherStage[slot] = nullptr; g.gatherCap[slot] = 0;
    HIP_OK(hipMalloc(&g.gatherStage[slot], std::max<size_t>(bytes, 16)));
    g.gatherCap[slot] = bytes;
    return 0;
}

// RD::TraceRays (radiance.cpp:242-267).  One device: the frame.  n devices (rdx_init_devices): the frame sharded by interleaved
// 64x64 tiles -- one internal host thread per device drives that device's streams, the caller's single blocking call returns
// when every shard is done and its RGBA8 + imageScratch tiles have been copied into device 0's buffers (peer copies over xGMI;
// no collective library is needed inside one process), where ReadBuffer reads them.
extern "C" int rdx_trace_rays(uint32_t, uint32_t, uint32_t, uint32_t width, uint32_t height)
{
    if (g_ndev <= 1) return trace_rays_device(width, height);
    if (!g0.initialized) return fail("rdx_init has not been called");
    if (g0.world > 1) return fail("TraceRays: rdx_set_shard and rdx_init_devices cannot be combined");
    if (g0.nslots < 14 || !g0.slots[13] || !known_buffer(g0.slots[13]) || !g0.slots[1] || !known_buffer(g0.slots[1]) ||
        !g0.slots[2] || !known_buffer(g0.slots[2]))
        return trace_rays_device(width, height);       // reports the binding error
    auto* bScratch = static_cast<rdx_buffer_s*>(g0.slots[1]);
    auto* bImage = static_cast<rdx_buffer_s*>(g0.slots[2]);
    auto* bTlas = static_cast<rdx_buffer_s*>(g0.slots[13]);
    const int n = g_ndev;
    // registry-side state each device context needs, and the derived traversal layout on every device (sequentially: the host
    // copy of the blob is shared)
    for (int d = 1; d < n; ++d) {
        Context& c = *g_dev[d];
        std::memcpy(c.slots, g0.slots, sizeof c.slots);
        c.nslots = g0.nslots; c.pipeline = g0.pipeline;
        c.opt = g0.opt;
    }
    for (int d = 0; d < n; ++d) {
        tl_ctx = g_dev[d]; tl_dev = d;
        hipError_t e = hipSetDevice(g_phys[d]);
        const int rc = e == hipSuccess ? derive_accel(bTlas) : -1;
        const std::string msg = g.err;
        tl_ctx = &g0; tl_dev = 0;
        HIP_IGN(hipSetDevice(g_phys[0]));
        if (rc) return fail("device %d: %s", d, e == hipSuccess ? msg.c_str() : hipGetErrorString(e));
    }
    std::vector<int> rcs(n, 0);
    std::vector<std::string> msgs(n);
    auto work = [&](int d) {
        tl_ctx = g_dev[d]; tl_dev = d;
        if (hipSetDevice(g_phys[d]) != hipSuccess) { rcs[d] = -1; msgs[d] = "hipSetDevice failed"; return; }
        g.rank = (uint32_t)d; g.world = (uint32_t)n; g.tileW = 64; g.tileH = 64;
        rcs[d] = trace_rays_device(width, height);
        if (rcs[d]) msgs[d] = g.err;
    };
    {
        std::vector<std::thread> pool;
        for (int d = 1; d < n; ++d) pool.emplace_back(work, d);
        work(0);
        for (auto& t : pool) t.join();
    }
    tl_ctx = &g0; tl_dev = 0;
    g0.rank = 0; g0.world = 1;
    HIP_OK(hipSetDevice(g_phys[0]));
    for (int d = 0; d < n; ++d) if (rcs[d]) return fail("device %d: %s", d, msgs[d].c_str());
    // gather: device d's tiles -> device 0 (image and the running-mean accumulator)
    const uint32_t tilesX = (width + 63) / 64, tilesY = (height + 63) / 64, nTiles = tilesX * tilesY;
    for (int d = 1; d < n; ++d) {
        const uint32_t owned = nTiles > (uint32_t)d ? (nTiles - d + n - 1) / n : 0;
        if (!owned) continue;
        const size_t bytes[2] = {(size_t)owned * 64 * 64 * 4, (size_t)owned * 64 * 64 * 16};
        const uint32_t elem[2] = {4, 16};
        rdx_buffer_s* src[2] = {bImage, bScratch};
        for (int k = 0; k < 2; ++k) {
            if (ensure_stage(2 + k, bytes[k])) return -1;                      // landing buffer on device 0
            void* land = g0.gatherStage[2 + k];
            tl_ctx = g_dev[d]; tl_dev = d;
            hipError_t e = hipSetDevice(g_phys[d]);
            int rc = e == hipSuccess ? ensure_stage(k, bytes[k]) : -1;
            void* stage = g.gatherStage[k];
            if (!rc) {
                launch_pack_tiles(g.stream, static_cast<uint8_t*>(src[k]->rep[d]), static_cast<uint8_t*>(stage), width, height, elem[k], 64, 64,
                                  (uint32_t)d, (uint32_t)n, false);
                e = hipGetLastError();
                if (e == hipSuccess) e = g_phys[d] == g_phys[0] ? hipMemcpyAsync(land, stage, bytes[k], hipMemcpyDeviceToDevice, g.stream)
                                                                : hipMemcpyPeerAsync(land, g_phys[0], stage, g_phys[d], bytes[k], g.stream);
                if (e == hipSuccess) e = hipStreamSynchronize(g.stream);
                if (e != hipSuccess) rc = -1;
            }
            const std::string msg = rc ? (e != hipSuccess ? std::string(hipGetErrorString(e)) : g.err) : std::string();
            tl_ctx = &g0; tl_dev = 0;
            HIP_IGN(hipSetDevice(g_phys[0]));
            if (rc) return fail("gather from device %d: %s", d, msg.c_str());
            launch_pack_tiles(g0.stream, static_cast<uint8_t*>(src[k]->dptr), static_cast<uint8_t*>(land), width, height, elem[k], 64, 64,
                              (uint32_t)d, (uint32_t)n, true);
            HIP_OK(hipGetLastError());
            HIP_OK(hipStreamSynchronize(g0.stream));
        }
    }
    // statistics of the whole frame: rays summed over the devices, times = the slowest device
    for (int d = 1; d < n; ++d) {
        const rdx_trace_stats& t = g_dev[d]->stats;
        rdx_trace_stats& a = g0.stats;
        a.rays_primary += t.rays_primary; a.rays_bounce += t.rays_bounce; a.rays_shadow += t.rays_shadow;
        a.closest_hits += t.closest_hits; a.pixels += t.pixels;
        a.ms_total = std::max(a.ms_total, t.ms_total);
        for (int i = 0; i < 65; ++i) g0.bounceCounts[i] += g_dev[d]->bounceCounts[i];
    }
    return 0;
}

// ------------------------------------------------------------------------------------------------
// test seams
// ------------------------------------------------------------------------------------------------
namespace {
template <class T> struct DevArray {
    T* p = nullptr;
    ~DevArray() { if (p) HIP_IGN(hipFree(p)); }
    hipError_t alloc(size_t n) { return hipMalloc(reinterpret_cast<void**>(&p), std::max<size_t>(n, 1) * sizeof(T)); }
    hipError_t upload(const T* src, size_t n) { hipError_t e = alloc(n); if (e != hipSuccess || !n) return e; return hipMemcpy(p, src, n * sizeof(T), hipMemcpyHostToDevice); }
};
}

extern "C" int rdx_trace_batch(rdx_buffer tlas, const float* o, const float* d, uint32_t n, float tmin, float tmax,
                               int rec, int mode, rdx_hit* out, uint64_t* visit4)
{
    if (mode != 0 && mode != 1) return fail("rdx_trace_batch: mode must be 0 (production) or 1 (reference order)");
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_batch: invalid TLAS handle");
    if (rec != 1 && rec != 2) return fail("rdx_trace_batch: sbtRecordOffset must be 1 or 2");
    if (derive_accel(tlas)) return -1;
    DevArray<float> dO, dD; DevArray<rdx_hit> dH;
    HIP_OK(dO.upload(o, 3 * (size_t)n)); HIP_OK(dD.upload(d, 3 * (size_t)n)); HIP_OK(dH.alloc(n));
    if (visit4) HIP_OK(hipMemsetAsync(g.dVisit, 0, 8 * sizeof(unsigned long long), g.stream));
    HIP_OK(hipMemsetAsync(g.dCounts + 64, 0, sizeof(uint32_t), g.stream));
    HIP_OK(hipEventRecord(g.evA, g.stream));
    launch_trace_batch(g.stream, view_of(tlas), dO.p, dD.p, n, tmin, tmax, rec, dH.p, visit4 ? g.dVisit : nullptr, mode, g.dCounts + 64);
    HIP_OK(hipEventRecord(g.evB, g.stream));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    if (take_status()) return fail("rdx_trace_batch: a traversal wave exceeded its iteration bound and gave up; the batch is incomplete");
    std::memset(&g.stats, 0, sizeof g.stats);
    HIP_OK(hipEventElapsedTime(&g.stats.ms_extend, g.evA, g.evB));      // kernel time of this batch
    if (n) HIP_OK(hipMemcpy(out, dH.p, (size_t)n * sizeof(rdx_hit), hipMemcpyDeviceToHost));
    if (visit4) {
        unsigned long long v[8];
        HIP_OK(hipMemcpy(v, g.dVisit, sizeof v, hipMemcpyDeviceToHost));
        for (int k = 0; k < 4; ++k) visit4[k] = v[(rec - 1) * 4 + k];
    }
    return 0;
}

// ---- what every device-resident call below shares -------------------------------------------------------------------
namespace {
// a byte range a kernel touches, as plain numbers: {address of the buffer, its size, offset, bytes, required multiple of offset and
// address, name, given at all}.  Nothing in the rule dereferences an address
struct RangeRow { uintptr_t addr; size_t size, off, bytes; uint32_t align; const char* name; bool present; };
bool ranges_overlap(const RangeRow& a, const RangeRow& b)
{
    if (!a.present || !b.present || !a.bytes || !b.bytes) return false;
    const uintptr_t a0 = a.addr + a.off, a1 = a0 + a.bytes, b0 = b.addr + b.off, b1 = b0 + b.bytes;
    return a0 < b1 && b0 < a1;
}
// The rule, in the order of its refusals: the offset of every present row, then every size (no sum that could wrap), then the
// caller's *_out words are zeroed and n == 0 is done; then the addresses (wrapped memory), the scene streams' (streamsAligned: the
// caller's finding), and the overlaps: outputs are R[firstOut ..], none may overlap a row before it, inputs may overlap each other
int check_ranges(const char* who, const RangeRow* R, int count, int firstOut, uint32_t n, std::initializer_list<uint32_t*> outWords = {},
                 bool streamsAligned = true)
{
    for (int k = 0; k < count; ++k)
        if (R[k].present && (R[k].off & (R[k].align - 1u)))
            return fail("%s: an offset must be a multiple of its range's alignment, %u for %s (offset %zu)", who, R[k].align, R[k].name, R[k].off);
    for (int k = 0; k < count; ++k)
        if (R[k].present && (R[k].off > R[k].size || R[k].bytes > R[k].size - R[k].off))
            return fail("%s: %u records at offset %zu run past the %s buffer (%zu bytes)", who, n, R[k].off, R[k].name, R[k].size);
    for (uint32_t* w : outWords) if (w) *w = 0;
    if (!n) return 0;
    for (int k = 0; k < count; ++k)
        if (R[k].present && (R[k].addr & (R[k].align - 1u)))
            return fail("%s: wrapped device memory must be %u-byte aligned (%s buffer)", who, R[k].align, R[k].name);
    if (!streamsAligned) return fail("%s: wrapped scene streams must be 4-byte aligned", who);
    for (int o = firstOut; o < count; ++o)
        for (int k = 0; k < o; ++k)
            if (ranges_overlap(R[o], R[k])) return fail("%s: the %s range and the %s range overlap", who, R[o].name, R[k].name);
    return 0;
}

// a call's table: one row per range, inputs first.  required: a NULL handle is refused, else it is an absent row
struct CallRange { rdx_buffer b; size_t off, bytes; const char* name; uint32_t align; bool required; };
constexpr size_t WHOLE_BUFFER = ~(size_t)0;     // as `bytes`: the row spans its buffer, whatever n is
template <int N> int check_call_handles(const char* who, const CallRange (&R)[N])
{
    for (int optional = 0; optional < 2; ++optional)       // the required rows first
        for (const CallRange& r : R)
            if (r.required != (optional != 0) && (r.b ? !known_buffer(r.b) : r.required)) return fail("%s: invalid %s buffer handle", who, r.name);
    return 0;
}
template <int N> int check_call_ranges(const char* who, const CallRange (&R)[N], int firstOut, uint32_t n,
                                       std::initializer_list<uint32_t*> outWords = {}, bool streamsAligned = true)
{
    RangeRow rows[N];
    for (int k = 0; k < N; ++k) {
        const rdx_buffer b = R[k].b;
        rows[k] = RangeRow{b ? reinterpret_cast<uintptr_t>(b->dptr) : 0, b ? b->size : 0, R[k].off, b && R[k].bytes == WHOLE_BUFFER ? b->size : R[k].bytes,
                           R[k].align, R[k].name, b != nullptr};
    }
    return check_ranges(who, rows, N, firstOut, n, outWords, streamsAligned);
}

template <class T> T* at(rdx_buffer b, size_t off = 0) { return b ? reinterpret_cast<T*>(static_cast<char*>(b->dptr) + off) : nullptr; }
bool aligned4(rdx_buffer b) { return !b || !(reinterpret_cast<uintptr_t>(b->dptr) & 3u); }
void mark_written(std::initializer_list<rdx_buffer> outs)      // device code wrote them
{
    for (rdx_buffer b : outs) if (b) { ++b->version; b->mirrorValid = false; }
}
// one launch on g.stream between the two events, waited for; its kernel time is the one figure of g.stats.  Counters are cleared
// before it and read back after it by the caller
template <class Launch> int timed_launch(float rdx_trace_stats::* ms, std::initializer_list<rdx_buffer> outs, Launch&& launch)
{
    HIP_OK(hipEventRecord(g.evA, g.stream));
    launch();
    HIP_OK(hipEventRecord(g.evB, g.stream));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    mark_written(outs);
    std::memset(&g.stats, 0, sizeof g.stats);
    HIP_OK(hipEventElapsedTime(&(g.stats.*ms), g.evA, g.evB));
    return 0;
}

// descriptor slots 5, 7, 8, 9 with their element counts; uv may be null
SurfaceScene surface_scene(rdx_buffer meshInfo, rdx_buffer index, rdx_buffer normal, rdx_buffer uv)
{
    SurfaceScene s{};
    s.meshInfo = at<const MeshInfo>(meshInfo); s.nMeshInfo = (uint32_t)std::min<size_t>(meshInfo->size / sizeof(MeshInfo), 0xffffffffu);
    s.index = at<const uint32_t>(index); s.nIndex = index->size / sizeof(uint32_t);
    s.normal = at<const float>(normal); s.nNormal = normal->size / sizeof(float);
    if (uv) { s.uv = at<const float>(uv); s.nUv = uv->size / sizeof(float); }
    return s;
}
int check_surface_handles(const char* who, const rdx_surface_buffers* scene)
{
    if (!scene) return fail("%s: no scene buffers", who);
    if (!scene->meshInfo || !known_buffer(scene->meshInfo)) return fail("%s: invalid meshInfo buffer handle", who);
    if (!scene->index || !known_buffer(scene->index)) return fail("%s: invalid index buffer handle", who);
    if (!scene->normal || !known_buffer(scene->normal)) return fail("%s: invalid normal buffer handle", who);
    if (scene->uv && !known_buffer(scene->uv)) return fail("%s: invalid uv buffer handle", who);
    return 0;
}
bool surface_aligned(const rdx_surface_buffers* s) { return aligned4(s->meshInfo) && aligned4(s->index) && aligned4(s->normal) && aligned4(s->uv); }
} // namespace

extern "C" int rdx_debug_check_ranges(const rdx_debug_range* rows, const char* const* names, uint32_t count, uint32_t first_out, uint32_t n)
{
    if (count && (!rows || !names)) return fail("rdx_debug_check_ranges: no rows");
    std::vector<RangeRow> R(count);
    for (uint32_t k = 0; k < count; ++k) {
        if (!rows[k].align || (rows[k].align & (rows[k].align - 1u))) return fail("rdx_debug_check_ranges: row %u: align %u is not a power of two", k, rows[k].align);
        R[k] = RangeRow{(uintptr_t)rows[k].address, (size_t)rows[k].size, (size_t)rows[k].offset, (size_t)rows[k].bytes, rows[k].align,
                        names[k] ? names[k] : "?", rows[k].present != 0};
    }
    return check_ranges("rdx_debug_check_ranges", R.data(), (int)count, (int)std::min<uint32_t>(first_out, count), n);
}

// Device-resident ray queries: nothing is staged through the host and nothing is allocated
extern "C" int rdx_query_rays(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, uint32_t n, int kind, rdx_buffer hits, size_t hits_offset)
{
    const char* who = "rdx_query_rays";
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_query_rays: invalid TLAS handle");
    static_assert(sizeof(rdx_ray) == 32 && sizeof(rdx_ray_hit) == 32, "two float4 per ray, two per record");
    const CallRange R[2] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {hits, hits_offset, (size_t)n * sizeof(rdx_ray_hit), "hit", 16, true}};
    if (check_call_handles(who, R)) return -1;
    if (kind != RDX_QUERY_CLOSEST && kind != RDX_QUERY_ANY) return fail("rdx_query_rays: kind must be RDX_QUERY_CLOSEST (1) or RDX_QUERY_ANY (2), not %d", kind);
    if (check_call_ranges(who, R, 1, n)) return -1;
    if (!n) return 0;
    if (derive_accel(tlas)) return -1;
    HIP_OK(hipMemsetAsync(g.dCounts + 64, 0, sizeof(uint32_t), g.stream));
    if (timed_launch(&rdx_trace_stats::ms_extend, {hits}, [&] {
            launch_query_rays(g.stream, view_of(tlas), at<const float4>(rays, rays_offset), n, kind, at<float4>(hits, hits_offset), g.dCounts + 64); }))
        return -1;
    if (take_status()) return fail("rdx_query_rays: a traversal wave exceeded its iteration bound and gave up; the batch is incomplete");
    return 0;
}

// Test seam of the per-bounce ray sort: the frame path's launch (group 0's scratch and phase) on the caller's keys
extern "C" int rdx_debug_sort_keys(rdx_buffer keys, size_t keys_offset, uint32_t live, uint32_t capacity, uint32_t key_bits, rdx_buffer perm,
                                   size_t perm_offset)
{
    const char* who = "rdx_debug_sort_keys";
    if (!g.initialized) return fail("rdx_init has not been called");
    const CallRange R[2] = {{keys, keys_offset, (size_t)capacity * sizeof(uint16_t), "key", 2, true},
                            {perm, perm_offset, (size_t)capacity * sizeof(uint32_t), "permutation", 4, true}};
    if (check_call_handles(who, R)) return -1;
    if (key_bits < 12u || key_bits > 14u) return fail("rdx_debug_sort_keys: key_bits must be 12, 13 or 14, not %u", key_bits);
    if (live > capacity) return fail("rdx_debug_sort_keys: %u live keys in a capacity of %u", live, capacity);
    if (capacity > (1u << 30)) return fail("rdx_debug_sort_keys: a capacity of %u keys is more than 2^30", capacity);
    if (check_call_ranges(who, R, 1, capacity)) return -1;
    if (!capacity) return 0;
    Context::Group& G = g.groups[0];
    if (ensure_sort_bins(G)) return -1;
    HIP_OK(hipMemcpy(G.dCounts + 1, &live, sizeof live, hipMemcpyHostToDevice));
    PathStreams ps{};
    ps.sortKey = at<unsigned short>(keys, keys_offset);
    return timed_launch(&rdx_trace_stats::ms_sort, {perm}, [&] {
        launch_ray_sort_tiles(g.stream, ps, G.dCounts + 1, capacity, SortBox{}, G.sortBins, G.sortPhase, at<uint32_t>(perm, perm_offset), key_bits); });
}

// Surface records of a query's hits (surface.hip)
extern "C" int rdx_resolve_hits(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer hits, size_t hits_offset, uint32_t n,
                                const rdx_surface_buffers* scene, rdx_buffer out, size_t out_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_resolve_hits";
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_resolve_hits: invalid TLAS handle");
    static_assert(sizeof(rdx_surface) == 64 && sizeof(MeshInfo) == sizeof(rdx_mesh_info), "four float4 per surface record");
    const CallRange R[3] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {hits, hits_offset, (size_t)n * sizeof(rdx_ray_hit), "hit", 16, true},
                            {out, out_offset, (size_t)n * sizeof(rdx_surface), "output", 16, true}};
    if (check_call_handles(who, R) || check_surface_handles(who, scene)) return -1;
    if (check_call_ranges(who, R, 2, n, {invalid_out}, surface_aligned(scene))) return -1;
    if (!n) return 0;
    if (derive_accel(tlas)) return -1;
    const AccelCache& ac = *acc(tlas);
    // (ShadeScene passes the uv stream only with textures on; here it is passed whenever it is given)
    const SurfaceScene sc = surface_scene(scene->meshInfo, scene->index, scene->normal, scene->uv && scene->uv->size >= sizeof(float) ? scene->uv : nullptr);
    HIP_OK(hipMemsetAsync(g.dSurfaceInvalid, 0, sizeof(uint32_t), g.stream));
    if (timed_launch(&rdx_trace_stats::ms_shade, {out}, [&] {
            launch_resolve_hits(g.stream, ac.insts, ac.slotOf, ac.s.nInst, at<const float4>(rays, rays_offset), at<const float4>(hits, hits_offset), n, sc,
                                at<float4>(out, out_offset), g.dSurfaceInvalid); }))
        return -1;
    uint32_t invalid = 0;
    HIP_OK(hipMemcpy(&invalid, g.dSurfaceInvalid, sizeof invalid, hipMemcpyDeviceToHost));
    if (invalid_out) *invalid_out = invalid;
    return 0;
}

extern "C" int rdx_debug_surface_in_bounds(const rdx_mesh_info* mi, uint32_t ninst, uint32_t nmeshinfo, uint32_t instanceIndex,
                                           uint32_t primitiveIndex, const uint32_t idx3[3], uint64_t nindex, uint64_t nnormal, uint64_t nuv)
{
    if (!mi) return fail("rdx_debug_surface_in_bounds: no MeshInfo records");
    return surface_in_bounds(reinterpret_cast<const MeshInfo*>(mi), ninst, nmeshinfo, instanceIndex, primitiveIndex, idx3, nindex, nnormal, nuv) ? 1 : 0;
}

// ---- an rdx_shading_buffers as rdx_shade_hits and rdx_trace_paths check it --------------------------------------------------
namespace {
// handles and the scene buffer's size; samplerBits = the sampler as TexView::flags bits (no sampler: repeat + nearest, as scene_args)
int check_shading_handles(const char* who, const rdx_shading_buffers* scene, uint32_t& samplerBits)
{
    if (!scene) return fail("%s: no scene buffers", who);
    if (!scene->scene || !known_buffer(scene->scene)) return fail("%s: invalid scene (SceneProperties) buffer handle", who);
    if (!scene->meshInfo || !known_buffer(scene->meshInfo)) return fail("%s: invalid meshInfo buffer handle", who);
    if (!scene->index || !known_buffer(scene->index)) return fail("%s: invalid index buffer handle", who);
    if (!scene->normal || !known_buffer(scene->normal)) return fail("%s: invalid normal buffer handle", who);
    if (!scene->material || !known_buffer(scene->material)) return fail("%s: invalid material buffer handle", who);
    if (scene->uv && !known_buffer(scene->uv)) return fail("%s: invalid uv buffer handle", who);
    if (scene->textureArray && !known_buffer(scene->textureArray)) return fail("%s: invalid textureArray handle", who);
    samplerBits = TEX_ADDR_REPEAT << TEX_ADDR_SHIFT;
    if (scene->sampler && !sampler_bits(scene->sampler, samplerBits)) return fail("%s: invalid sampler handle", who);
    if (scene->scene->size < sizeof(SceneProperties))
        return fail("%s: the scene buffer (%zu bytes) does not hold a SceneProperties (%zu bytes)", who, scene->scene->size, sizeof(SceneProperties));
    return 0;
}
bool shading_aligned(const rdx_shading_buffers* s)
{
    return aligned4(s->scene) && aligned4(s->meshInfo) && aligned4(s->index) && aligned4(s->normal) && aligned4(s->material) && aligned4(s->uv) &&
           aligned4(s->textureArray);
}
// the stock shader's rule (scene_args): texels are read only when option "textures" is 1 and an image array is given; the uv
// buffer is required then
int shading_textures(const char* who, const rdx_shading_buffers* scene, uint32_t samplerBits, TexView& tex)
{
    tex = TexView{nullptr, 0, 0, 0, 0};
    if (!g.opt.textures || !scene->textureArray) return 0;
    const rdx_buffer_s* img = scene->textureArray;
    if (!img->imgW || !img->imgH || !img->imgLayers) return fail("%s: textureArray is not an image array (rdx_image_array_create)", who);
    if (img->size / 4 / img->imgW / img->imgH < img->imgLayers) return fail("%s: textureArray is smaller than its %u layers", who, img->imgLayers);
    if (!scene->uv || scene->uv->size < sizeof(float)) return fail("%s: option \"textures\" is 1 and a textureArray is given, but no uv buffer", who);
    tex = TexView{static_cast<const uint8_t*>(img->dptr), img->imgW, img->imgH, img->imgLayers, TEX_ENABLED | samplerBits};
    return 0;
}
// the scene as shade.hip, material.hip and light_paths.hip read it: the pointers, the element counts, the texture view, and the uv
// stream only with textures on
int shade_scene(const char* who, const rdx_shading_buffers* scene, uint32_t samplerBits, ShadeScene& sc)
{
    sc = ShadeScene{};
    sc.scene = at<const SceneProperties>(scene->scene);
    sc.materials = at<const Material>(scene->material); sc.nMaterials = (uint32_t)std::min<size_t>(scene->material->size / sizeof(Material), 0xffffffffu);
    if (shading_textures(who, scene, samplerBits, sc.tex)) return -1;
    sc.s = surface_scene(scene->meshInfo, scene->index, scene->normal, (sc.tex.flags & TEX_ENABLED) ? scene->uv : nullptr);
    return 0;
}
} // namespace

// The stock closest-hit / miss shaders on a query's records (shade.hip)
extern "C" int rdx_shade_hits(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer hits, size_t hits_offset, rdx_buffer keys,
                              size_t keys_offset, uint32_t n, const rdx_shading_buffers* scene, rdx_buffer shade, size_t shade_offset,
                              rdx_buffer next, size_t next_offset, rdx_buffer shadow, size_t shadow_offset, rdx_buffer src, size_t src_offset,
                              uint32_t* live_out, uint32_t* invalid_out)
{
    const char* who = "rdx_shade_hits";
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_shade_hits: invalid TLAS handle");
    static_assert(sizeof(rdx_shade) == 48 && sizeof(rdx_shade_key) == 16 && sizeof(rdx_shading_buffers) == 8 * sizeof(void*), "three float4 per shade record, one uint4 per key");
    // the first three are read, the others written; src is held to 16 bytes here (4 in rdx_scatter_hits)
    const CallRange R[7] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {hits, hits_offset, (size_t)n * sizeof(rdx_ray_hit), "hit", 16, true},
                            {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true}, {shade, shade_offset, (size_t)n * sizeof(rdx_shade), "shade", 16, true},
                            {next, next_offset, (size_t)n * sizeof(rdx_ray), "next-ray", 16, false}, {shadow, shadow_offset, (size_t)n * sizeof(rdx_ray), "shadow-ray", 16, false},
                            {src, src_offset, (size_t)n * sizeof(uint32_t), "src", 16, false}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (check_call_ranges(who, R, 3, n, {live_out, invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    const AccelCache& ac = *acc(tlas);
    HIP_OK(hipMemsetAsync(g.dShadeCounts, 0, 2 * sizeof(uint32_t), g.stream));
    if (timed_launch(&rdx_trace_stats::ms_shade, {shade, next, shadow, src}, [&] {
            launch_shade_hits(g.stream, ac.insts, ac.slotOf, ac.s.nInst, at<const float4>(rays, rays_offset), at<const float4>(hits, hits_offset),
                              at<const uint4>(keys, keys_offset), n, sc, at<float4>(shade, shade_offset), at<float4>(next, next_offset),
                              at<float4>(shadow, shadow_offset), at<uint32_t>(src, src_offset), g.dShadeCounts, g.dShadeCounts + 1); }))
        return -1;
    uint32_t counts[2] = {0, 0};
    HIP_OK(hipMemcpy(counts, g.dShadeCounts, sizeof counts, hipMemcpyDeviceToHost));
    if (live_out) *live_out = counts[0];
    if (invalid_out) *invalid_out = counts[1];
    return 0;
}

extern "C" int rdx_debug_shade_in_bounds(const rdx_mesh_info* mi, uint32_t ninst, uint32_t nmeshinfo, uint32_t instanceIndex,
                                         uint32_t primitiveIndex, const uint32_t idx3[3], uint64_t nindex, uint64_t nnormal, uint64_t nuv,
                                         const rdx_material* materials, uint32_t nmaterials, int textures, uint32_t layers)
{
    if (!mi) return fail("rdx_debug_shade_in_bounds: no MeshInfo records");
    if (!materials && nmaterials) return fail("rdx_debug_shade_in_bounds: no Material records");
    static_assert(sizeof(Material) == sizeof(rdx_material), "Material layout");
    return shade_in_bounds(reinterpret_cast<const MeshInfo*>(mi), ninst, nmeshinfo, instanceIndex, primitiveIndex, idx3, nindex, nnormal,
                           textures ? nuv : 0u, reinterpret_cast<const Material*>(materials), nmaterials, textures != 0, layers) ? 1 : 0;
}

// The evaluated material of a query's hits (material.hip): the inputs are those of rdx_shade_hits without the keys
extern "C" int rdx_resolve_materials(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer hits, size_t hits_offset, uint32_t n,
                                     const rdx_shading_buffers* scene, rdx_buffer out, size_t out_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_resolve_materials";
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_resolve_materials: invalid TLAS handle");
    static_assert(sizeof(rdx_material_record) == 64, "four float4 per material record");
    const CallRange R[3] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {hits, hits_offset, (size_t)n * sizeof(rdx_ray_hit), "hit", 16, true},
                            {out, out_offset, (size_t)n * sizeof(rdx_material_record), "output", 16, true}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (check_call_ranges(who, R, 2, n, {invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    const AccelCache& ac = *acc(tlas);
    HIP_OK(hipMemsetAsync(g.dShadeCounts, 0, 2 * sizeof(uint32_t), g.stream));
    if (timed_launch(&rdx_trace_stats::ms_shade, {out}, [&] {
            launch_resolve_materials(g.stream, ac.insts, ac.slotOf, ac.s.nInst, at<const float4>(rays, rays_offset), at<const float4>(hits, hits_offset), n, sc,
                                     at<float4>(out, out_offset), g.dShadeCounts + 1); }))
        return -1;
    uint32_t invalid = 0;
    HIP_OK(hipMemcpy(&invalid, g.dShadeCounts + 1, sizeof invalid, hipMemcpyDeviceToHost));
    if (invalid_out) *invalid_out = invalid;
    return 0;
}

// One directional light's direct term on material records (material.hip).  No TLAS and no scene streams: the kernel reads the
// rays' directions, the records and the one DirLight, so the checks are those of the ranges alone
extern "C" int rdx_light_hits(rdx_buffer rays, size_t rays_offset, rdx_buffer materials, size_t materials_offset, uint32_t n, rdx_buffer scene,
                              uint32_t light, rdx_buffer lit, size_t lit_offset, rdx_buffer shadow, size_t shadow_offset)
{
    const char* who = "rdx_light_hits";
    if (!g.initialized) return fail("rdx_init has not been called");
    // the first three are read (the whole SceneProperties stands for its one light), the others written
    const CallRange R[5] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true},
                            {materials, materials_offset, (size_t)n * sizeof(rdx_material_record), "material-record", 16, true},
                            {scene, 0, sizeof(SceneProperties), "scene (SceneProperties)", 4, true},
                            {lit, lit_offset, (size_t)n * 4 * sizeof(float), "lit", 16, true}, {shadow, shadow_offset, (size_t)n * sizeof(rdx_ray), "shadow-ray", 16, false}};
    if (check_call_handles(who, R)) return -1;
    constexpr uint32_t nLights = sizeof(SceneProperties::lights) / sizeof(DirLight);
    if (light >= nLights) return fail("rdx_light_hits: light %u is not one of the %u lights of a SceneProperties (0 .. %u)", light, nLights, nLights - 1u);
    if (scene->size < sizeof(SceneProperties))
        return fail("rdx_light_hits: the scene buffer (%zu bytes) does not hold a SceneProperties (%zu bytes)", scene->size, sizeof(SceneProperties));
    if (check_call_ranges(who, R, 3, n)) return -1;
    if (!n) return 0;
    return timed_launch(&rdx_trace_stats::ms_shade, {lit, shadow}, [&] {
        launch_light_hits(g.stream, at<const float4>(rays, rays_offset), at<const float4>(materials, materials_offset), n,
                          at<const DirLight>(scene, offsetof(SceneProperties, lights)) + light, at<float4>(lit, lit_offset), at<float4>(shadow, shadow_offset)); });
}

// The next-direction sample of `material` on material and surface records (scatter.hip).  No TLAS and no scene buffers: the kernel
// reads the rays' directions, the records and one key or one float4 of randoms per ray, so the checks are those of the ranges
// alone.  *live is the counter word of rdx_shade_hits
extern "C" int rdx_scatter_hits(rdx_buffer rays, size_t rays_offset, rdx_buffer materials, size_t materials_offset, rdx_buffer surfaces,
                                size_t surfaces_offset, rdx_buffer keys, size_t keys_offset, rdx_buffer randoms, size_t randoms_offset, uint32_t n,
                                rdx_buffer scatter, size_t scatter_offset, rdx_buffer next, size_t next_offset, rdx_buffer src, size_t src_offset,
                                uint32_t* live_out)
{
    const char* who = "rdx_scatter_hits";
    if (!g.initialized) return fail("rdx_init has not been called");
    static_assert(sizeof(rdx_scatter) == 16 && sizeof(rdx_material_record) == 64 && sizeof(rdx_surface) == 64, "one float4 per scatter record");
    // the first five are read, the others written
    const CallRange R[8] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true},
                            {materials, materials_offset, (size_t)n * sizeof(rdx_material_record), "material-record", 16, true},
                            {surfaces, surfaces_offset, (size_t)n * sizeof(rdx_surface), "surface-record", 16, true},
                            {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, false}, {randoms, randoms_offset, (size_t)n * 4 * sizeof(float), "randoms", 16, false},
                            {scatter, scatter_offset, (size_t)n * sizeof(rdx_scatter), "scatter", 16, true}, {next, next_offset, (size_t)n * sizeof(rdx_ray), "next-ray", 16, true},
                            {src, src_offset, (size_t)n * sizeof(uint32_t), "src", 4, false}};
    if (check_call_handles(who, R)) return -1;
    if (!keys && !randoms) return fail("rdx_scatter_hits: neither keys nor randoms given: one of the two is required");
    if (keys && randoms) return fail("rdx_scatter_hits: both keys and randoms given: only one of the two is allowed");
    if (check_call_ranges(who, R, 5, n, {live_out})) return -1;
    if (!n) return 0;
    HIP_OK(hipMemsetAsync(g.dShadeCounts, 0, sizeof(uint32_t), g.stream));
    if (timed_launch(&rdx_trace_stats::ms_shade, {scatter, next, src}, [&] {
            launch_scatter_hits(g.stream, at<const float4>(rays, rays_offset), at<const float4>(materials, materials_offset), at<const float4>(surfaces, surfaces_offset),
                                at<const uint4>(keys, keys_offset), at<const float4>(randoms, randoms_offset), n, at<float4>(scatter, scatter_offset),
                                at<float4>(next, next_offset), at<uint32_t>(src, src_offset), g.dShadeCounts); }))
        return -1;
    uint32_t live = 0;
    HIP_OK(hipMemcpy(&live, g.dShadeCounts, sizeof live, hipMemcpyDeviceToHost));
    if (live_out) *live_out = live;
    return 0;
}

// ---- the two ends of a frame on device memory (raygen.hip) ---------------------------------------------------------------------
// Primary rays of the camera in `camera`, as rdx_ray / rdx_shade_key records on the device (include/rdx.h)
extern "C" int rdx_generate_rays(rdx_buffer camera, uint32_t n, uint32_t first_pixel, rdx_buffer pixels, size_t pixels_offset, uint32_t frameID,
                                 uint32_t totalSamples, rdx_buffer seeds, size_t seeds_offset, float tmin, float tmax, rdx_buffer rays,
                                 size_t rays_offset, rdx_buffer keys, size_t keys_offset)
{
    const char* who = "rdx_generate_rays";
    if (!g.initialized) return fail("rdx_init has not been called");
    static_assert(sizeof(rdx_raygen_seed) == 16 && sizeof(rdx_shade_key) == 16 && sizeof(rdx_ray) == 32, "one uint4 per seed and key, two float4 per ray");
    const CallRange R[5] = {{camera, 0, sizeof(PhysicalCamera), "camera", 4, true}, {pixels, pixels_offset, (size_t)n * sizeof(uint32_t), "pixel", 4, false},
                            {seeds, seeds_offset, (size_t)n * sizeof(rdx_raygen_seed), "seed", 16, false},
                            {rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, false}};
    if (check_call_handles(who, R)) return -1;
    if (camera->size < sizeof(PhysicalCamera))
        return fail("rdx_generate_rays: the camera buffer (%zu bytes) does not hold a PhysicalCamera (%zu bytes)", camera->size, sizeof(PhysicalCamera));
    if (!pixels && (uint64_t)first_pixel + n > 0x100000000ull)
        return fail("rdx_generate_rays: first_pixel + n (%u + %u) does not fit 32 bits", first_pixel, n);
    if (check_call_ranges(who, R, 3, n)) return -1;
    if (!n) return 0;
    // (the time includes the camera's one-thread kernel)
    return timed_launch(&rdx_trace_stats::ms_generate, {rays, keys}, [&] {
        launch_generate_rays(g.stream, at<const PhysicalCamera>(camera), g.dRaygenArgs, n, first_pixel, at<const uint32_t>(pixels, pixels_offset), frameID,
                             totalSamples, at<const uint4>(seeds, seeds_offset), tmin, tmax, at<float4>(rays, rays_offset), at<uint4>(keys, keys_offset)); });
}

// One sample per pixel folded into imageScratch, and the RGBA8 image of the new mean (include/rdx.h)
extern "C" int rdx_accumulate(rdx_buffer colors, size_t colors_offset, uint32_t n, uint32_t first_pixel, rdx_buffer pixels, size_t pixels_offset,
                              uint32_t frameID, rdx_buffer scratch, rdx_buffer image, uint32_t flags, uint32_t* invalid_out)
{
    const char* who = "rdx_accumulate";
    if (!g.initialized) return fail("rdx_init has not been called");
    const CallRange R[4] = {{colors, colors_offset, (size_t)n * sizeof(float4), "colour", 16, true}, {pixels, pixels_offset, (size_t)n * sizeof(uint32_t), "pixel", 4, false},
                            {scratch, 0, WHOLE_BUFFER, "scratch", 16, true}, {image, 0, WHOLE_BUFFER, "image", 4, false}};
    if (check_call_handles(who, R)) return -1;
    if (flags & ~1u) return fail("rdx_accumulate: unknown flags 0x%x (bit 0 = debug)", flags);
    if (!pixels && (uint64_t)first_pixel + n > 0x100000000ull)
        return fail("rdx_accumulate: first_pixel + n (%u + %u) does not fit 32 bits", first_pixel, n);
    if (check_call_ranges(who, R, 2, n, {invalid_out})) return -1;
    if (!n) return 0;
    // the frame: whole pixels both buffers hold
    size_t npix = scratch->size / sizeof(float4);
    if (image) npix = std::min(npix, image->size / 4);
    npix = std::min<size_t>(npix, 0xffffffffu);
    HIP_OK(hipMemsetAsync(g.dAccumInvalid, 0, sizeof(uint32_t), g.stream));
    if (timed_launch(&rdx_trace_stats::ms_accumulate, {scratch, image}, [&] {
            launch_accumulate_samples(g.stream, at<const float4>(colors, colors_offset), n, first_pixel, at<const uint32_t>(pixels, pixels_offset), frameID,
                                      at<float4>(scratch), at<uchar4>(image), (uint32_t)npix, flags & 1u, g.dAccumInvalid); }))
        return -1;
    uint32_t invalid = 0;
    HIP_OK(hipMemcpy(&invalid, g.dAccumInvalid, sizeof invalid, hipMemcpyDeviceToHost));
    if (invalid_out) *invalid_out = invalid;
    return 0;
}

// Radiance along the caller's own rays (include/rdx.h): launch_query_rays for the first segment, k_paths_ingest (paths.hip) to
// make paths of rays, records and keys, then the bounces of the frame path (trace_bounces) -- per chunk of "chunk_paths" paths, in
// group 0's streams.  A finished path stores its colour as record `slot` of sampleColor (BounceArgs: nPixels 0, sampleBase 0),
// which is the chunk's part of the caller's radiance range.
extern "C" int rdx_trace_paths(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n,
                               uint32_t max_depth, const rdx_shading_buffers* scene, rdx_buffer radiance, size_t radiance_offset,
                               rdx_buffer hits, size_t hits_offset)
{
    const char* who = "rdx_trace_paths";
    if (!g.initialized) return fail("rdx_trace_paths: rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_paths: invalid TLAS handle");
    static_assert(sizeof(rdx_ray) == 32 && sizeof(rdx_ray_hit) == 32 && sizeof(rdx_shade_key) == 16, "two float4 per ray and record, one uint4 per key");
    const CallRange R[4] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true},
                            {hits, hits_offset, (size_t)n * sizeof(rdx_ray_hit), "hit", 16, false}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (max_depth > 62) return fail("rdx_trace_paths: depth %u exceeds the supported maximum of 62", max_depth);
    if (check_call_ranges(who, R, 2, n, {}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    SceneArgs sc{};
    sc.scene = at<const SceneProperties>(scene->scene);
    sc.meshInfo = at<const MeshInfo>(scene->meshInfo);
    sc.indexData = at<const uint32_t>(scene->index);
    sc.uvData = at<const float>(scene->uv);
    sc.normalData = at<const float>(scene->normal);
    sc.materials = at<const Material>(scene->material);
    if (shading_textures(who, scene, samplerBits, sc.tex)) return -1;
    if (derive_accel(tlas)) return -1;
    const AccelCache& ac = *acc(tlas);

    const uint32_t chunk = (uint32_t)std::min<int64_t>(n, g.opt.chunkPaths);
    Context::Group& G = g.groups[0];
    if (max_depth && ensure_group(G, chunk)) return -1;
    if (max_depth && !hits && g.pathHitsCap < chunk) {
        if (g.pathHits) HIP_IGN(hipFree(g.pathHits));
        g.pathHits = nullptr; g.pathHitsCap = 0;
        HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.pathHits), (size_t)chunk * sizeof(rdx_ray_hit)));
        g.pathHitsCap = chunk;
    }
    const float4* dRays = at<const float4>(rays, rays_offset);
    const uint4* dKeys = at<const uint4>(keys, keys_offset);
    float4* dRad = at<float4>(radiance, radiance_offset);
    float4* dHits = at<float4>(hits, hits_offset);

    std::memset(&g.stats, 0, sizeof g.stats);
    std::memset(g.bounceCounts, 0, sizeof g.bounceCounts);
    g.stats.pixels = n;
    g.stats.groups = 1;
    g.visitDepth = 0;
    set_grid_share(1);
    // the first segment: the per-ray-interval engine on the view rdx_query_rays gives it; the bounces: the frame path's view
    const AccelView avQuery = view_of(tlas);
    BounceArgs B{tlas, view_of(tlas, (uint64_t)chunk <= (uint64_t)g.opt.sortMinPaths), sc, max_depth, 0u, 0u, false, false, false, SortBox{}, nullptr,
                 0.001f, 1000.0f};      // shader.cl:235-236, 500
    bounce_switches(chunk, B);
    B.overlap = false;
    HIP_OK(hipEventRecord(g.evA, g.stream));
    for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t m = std::min(chunk, n - c0);
        float4* segHits = dHits ? dHits + 2 * (size_t)c0 : g.pathHits;
        if (max_depth == 0) {
            // no segment is traced: colour 0 for every path; `hits` still gets the records of the query it stands for
            HIP_OK(hipMemsetAsync(dRad + c0, 0, (size_t)m * sizeof(float4), g.stream));
            if (dHits) {
                HIP_OK(hipMemsetAsync(G.dCounts + 64, 0, sizeof(uint32_t), g.stream));
                launch_query_rays(g.stream, avQuery, dRays + 2 * (size_t)c0, m, RDX_QUERY_CLOSEST, segHits, G.dCounts + 64);
            }
            continue;
        }
        std::memset(G.hCounts, 0, 256 * sizeof(uint32_t));
        G.hCounts[0] = m;
        HIP_OK(hipMemcpyAsync(G.dCounts, G.hCounts, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, G.s0));
        g_timer.begin(&g.stats.ms_extend, G.s0);
        launch_query_rays(G.s0, avQuery, dRays + 2 * (size_t)c0, m, RDX_QUERY_CLOSEST, segHits, G.dCounts + 64);
        g_timer.end(G.s0);
        g.stats.launches_extend++;
        PathStreams ps = G.ps;
        ps.sampleColor = dRad + c0;
        g_timer.begin(&g.stats.ms_generate, G.s0);
        launch_paths_ingest(G.s0, ac.slotOf, ac.s.nInst, dRays + 2 * (size_t)c0, segHits, dKeys + c0, m, ps);
        g_timer.end(G.s0);
        if (trace_bounces(B, &ps, &m, 1)) return -1;
        HIP_OK(hipMemcpyAsync(G.hCounts, G.dCounts, 256 * sizeof(uint32_t), hipMemcpyDeviceToHost, G.s0));
        HIP_OK(hipStreamSynchronize(g.stream));
        add_group_counts(1, max_depth);
    }
    HIP_OK(hipEventRecord(g.evB, g.stream));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    mark_written({radiance, hits});
    if (take_status()) return fail("rdx_trace_paths: a traversal wave exceeded its iteration bound and gave up; the batch is incomplete");
    HIP_OK(hipEventElapsedTime(&g.stats.ms_total, g.evA, g.evB));
    g_timer.resolve();
    return 0;
}

// The bounces of rdx_trace_paths_lights, rdx_trace_paths_punctual and rdx_trace_paths_area, after their checks (include/rdx.h;
// light_paths.hip, punctual.hip, area.hip).
// Per chunk of paths and per depth: launch_query_rays (closest) -> `shade`, the call's shade kernel over its L lights ->
// launch_query_rays (any) on the live x L shadow rays, one contiguous range, each under its own interval -> k_lights_fold.
// launch_query_rays sizes its grid on the host, so ONE word -- the survivors of the depth -- is read back per bounce; nothing else
// passes through the host.  The chunk's streams are one allocation that grows on first use and is reused: 192 + 80 L bytes per path
// (DESIGN 4.15, 4.16).
// `fold` is the call's fold kernel beside its shade kernel: k_lights_fold for all but rdx_trace_paths_env_mis, whose own hands the
// weight's fourth word on (env_mis.hip).
namespace {
using FoldLaunch = void (*)(hipStream_t, const float4*, uint32_t, const LightPathStreams&, uint32_t);
template <class ShadeLaunch>
int trace_light_paths(const char* who, rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n,
                      uint32_t max_depth, uint32_t L, const ShadeScene& sc, rdx_buffer radiance, size_t radiance_offset, uint32_t* invalid_out,
                      ShadeLaunch&& shade, FoldLaunch fold = launch_lights_fold)
{
    const AccelCache& ac = *acc(tlas);
    // a chunk's shadow rays are one launch_query_rays range, whose count is 32 bits; beyond the five lights of a SceneProperties a
    // chunk shrinks so that its streams are no larger than five lights' (592 bytes per path): no shorter for L <= 5
    const int64_t chunkPaths = std::min<int64_t>(g.opt.chunkPaths, 0xffffffffll);
    const uint32_t chunk = (uint32_t)std::min<int64_t>(std::min<int64_t>(std::min<int64_t>(n, chunkPaths), std::max<int64_t>(chunkPaths * 592 / (192 + 80 * (int64_t)L), 1)),
                                                       0xffffffffll / std::max<uint32_t>(L, 1u));
    Context::Group& G = g.groups[0];
    // the chunk's streams, each a multiple of 256 bytes: hits 32 | rays x 2 64 | ids x 2 32 | weight x 2 32 | foldF 16 | foldA 16 |
    // lit 16 L | shadow 32 L | any 32 L
    const size_t c256 = ((size_t)chunk + 15) & ~(size_t)15;
    if (max_depth) {
        const size_t need = c256 * (192 + 80 * (size_t)L);
        if (g.lightScratchCap < need) {
            if (g.lightScratch) HIP_IGN(hipFree(g.lightScratch));
            g.lightScratch = nullptr; g.lightScratchCap = 0;
            HIP_OK(hipMalloc(reinterpret_cast<void**>(&g.lightScratch), need));
            g.lightScratchCap = need;
        }
    }
    char* cursor = g.lightScratch;
    auto take = [&](size_t bytesPerPath) { char* p = cursor; cursor += c256 * bytesPerPath; return p; };
    float4* sHits = reinterpret_cast<float4*>(take(32));
    float4* sRays[2] = {reinterpret_cast<float4*>(take(32)), reinterpret_cast<float4*>(take(32))};
    uint4* sIds[2] = {reinterpret_cast<uint4*>(take(16)), reinterpret_cast<uint4*>(take(16))};
    float4* sWeight[2] = {reinterpret_cast<float4*>(take(16)), reinterpret_cast<float4*>(take(16))};
    float4* sFoldF = reinterpret_cast<float4*>(take(16));
    float4* sFoldA = reinterpret_cast<float4*>(take(16));
    float4* sLit = reinterpret_cast<float4*>(take(16 * (size_t)L));
    float4* sShadow = reinterpret_cast<float4*>(take(32 * (size_t)L));
    float4* sAny = reinterpret_cast<float4*>(take(32 * (size_t)L));

    const float4* dRays = at<const float4>(rays, rays_offset);
    const uint4* dKeys = at<const uint4>(keys, keys_offset);
    float4* dRad = at<float4>(radiance, radiance_offset);

    std::memset(&g.stats, 0, sizeof g.stats);
    std::memset(g.bounceCounts, 0, sizeof g.bounceCounts);
    g.stats.pixels = n;
    g.stats.groups = 1;
    g.visitDepth = 0;
    set_grid_share(1);
    const AccelView av = view_of(tlas);      // the per-ray-interval engine on the view rdx_query_rays gives it
    HIP_OK(hipMemsetAsync(g.dShadeCounts, 0, 2 * sizeof(uint32_t), g.stream));
    HIP_OK(hipEventRecord(g.evA, g.stream));
    for (uint32_t c0 = 0; c0 < n; c0 += chunk) {
        const uint32_t m = std::min(chunk, n - c0);
        if (max_depth == 0) {       // no segment is traced: colour 0 for every path
            HIP_OK(hipMemsetAsync(dRad + c0, 0, (size_t)m * sizeof(float4), g.stream));
            continue;
        }
        // G.dCounts: [d + 1] = survivors of depth d (the compaction cursor), [64 + d] / [128 + d] = the work counters of the depth's
        // closest-hit / any-hit launch, all zero before the first launch
        std::memset(G.hCounts, 0, 256 * sizeof(uint32_t));
        G.hCounts[0] = m;
        HIP_OK(hipMemcpyAsync(G.dCounts, G.hCounts, 256 * sizeof(uint32_t), hipMemcpyHostToDevice, G.s0));
        uint32_t liveRays = m;
        g.bounceCounts[0] += m;
        for (uint32_t d = 0; d < max_depth && liveRays; ++d) {
            const bool last = d + 1 == max_depth;
            LightPathStreams io{};
            io.rays = d == 0 ? dRays + 2 * (size_t)c0 : sRays[(d - 1) & 1u];
            io.hits = sHits;
            io.keys = d == 0 ? dKeys + c0 : nullptr;
            io.ids = d == 0 ? nullptr : sIds[(d - 1) & 1u];
            io.weight = d == 0 ? nullptr : sWeight[(d - 1) & 1u];
            io.nIds = sIds[d & 1u]; io.nWeight = sWeight[d & 1u]; io.nRays = sRays[d & 1u];
            io.foldF = sFoldF; io.foldA = sFoldA; io.lit = sLit; io.shadow = sShadow;
            io.radiance = dRad + c0;
            g_timer.begin(&g.stats.ms_extend, G.s0);
            launch_query_rays(G.s0, av, io.rays, liveRays, RDX_QUERY_CLOSEST, sHits, G.dCounts + 64 + d);
            g_timer.end(G.s0);
            g.stats.launches_extend++;
            g_timer.begin(&g.stats.ms_shade, G.s0);
            shade(G.s0, ac, io, liveRays, d, !last, G.dCounts + d + 1, g.dShadeCounts + 1);
            g_timer.end(G.s0);
            // the one word per bounce: launch_query_rays and the fold are sized on the host
            HIP_OK(hipMemcpyAsync(G.hCounts + d + 1, G.dCounts + d + 1, sizeof(uint32_t), hipMemcpyDeviceToHost, G.s0));
            HIP_OK(hipStreamSynchronize(G.s0));
            const uint32_t survivors = G.hCounts[d + 1];
            if (survivors > liveRays) return fail("%s: internal error: %u survivors of %u live rays", who, survivors, liveRays);
            if (survivors && L) {
                g_timer.begin(&g.stats.ms_shadow, G.s0);
                launch_query_rays(G.s0, av, sShadow, survivors * L, RDX_QUERY_ANY, sAny, G.dCounts + 128 + d);
                g_timer.end(G.s0);
                g.stats.launches_shadow++;
            }
            g_timer.begin(&g.stats.ms_shade, G.s0);
            fold(G.s0, sAny, L, io, survivors);
            g_timer.end(G.s0);
            g.bounceCounts[d + 1] += survivors;
            if (d == 0) g.stats.rays_primary += liveRays; else g.stats.rays_bounce += liveRays;
            g.stats.closest_hits += survivors;
            g.stats.rays_shadow += (uint64_t)L * survivors;
            liveRays = survivors;
        }
    }
    HIP_OK(hipEventRecord(g.evB, g.stream));
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    mark_written({radiance});
    if (take_status()) return fail("%s: a traversal wave exceeded its iteration bound and gave up; the batch is incomplete", who);
    uint32_t invalid = 0;
    HIP_OK(hipMemcpy(&invalid, g.dShadeCounts + 1, sizeof invalid, hipMemcpyDeviceToHost));
    if (invalid_out) *invalid_out = invalid;
    HIP_OK(hipEventElapsedTime(&g.stats.ms_total, g.evA, g.evB));
    g_timer.resolve();
    return 0;
}
} // namespace

// Radiance along the caller's own rays with every light of the scene sampled at every hit (include/rdx.h; light_paths.hip): the
// checks, then trace_light_paths with k_lights_shade over the DirLights of the SceneProperties
extern "C" int rdx_trace_paths_lights(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n,
                                      uint32_t max_depth, uint32_t light_count, const rdx_shading_buffers* scene, rdx_buffer radiance,
                                      size_t radiance_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_trace_paths_lights";
    if (!g.initialized) return fail("rdx_trace_paths_lights: rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_paths_lights: invalid TLAS handle");
    // the SceneProperties is a row because the kernels of every depth read its lights: optional here only so that a NULL `scene` or
    // a NULL handle in it is left to check_shading_handles
    const CallRange R[4] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true},
                            {scene ? scene->scene : nullptr, 0, sizeof(SceneProperties), "scene (SceneProperties)", 4, false},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (max_depth > 62) return fail("rdx_trace_paths_lights: depth %u exceeds the supported maximum of 62", max_depth);
    if (light_count > 5) return fail("rdx_trace_paths_lights: light_count %u exceeds the 5 lights of a SceneProperties", light_count);
    static_assert(sizeof(((SceneProperties*)nullptr)->lights) == 5 * sizeof(DirLight), "five DirLights");
    if (check_call_ranges(who, R, 3, n, {invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    const DirLight* lights = sc.scene->lights;       // a device address: read by the kernels of every call
    return trace_light_paths(who, tlas, rays, rays_offset, keys, keys_offset, n, max_depth, light_count, sc, radiance, radiance_offset, invalid_out,
                             [&](hipStream_t st, const AccelCache& ac, const LightPathStreams& io, uint32_t live, uint32_t d, bool sampleNext, uint32_t* cursor,
                                 uint32_t* invalid) {
                                 launch_lights_shade(st, ac.insts, ac.slotOf, ac.s.nInst, sc, lights, light_count, io, live, d, sampleNext, cursor, invalid); });
}

// One record of a caller's light table on material records (punctual.hip).  As rdx_light_hits: no TLAS and no scene streams, so the
// checks are those of the ranges alone; the one record stands in the table at light_offset
extern "C" int rdx_punctual_light_hits(rdx_buffer rays, size_t rays_offset, rdx_buffer materials, size_t materials_offset, uint32_t n, rdx_buffer lights,
                                       size_t light_offset, rdx_buffer lit, size_t lit_offset, rdx_buffer shadow, size_t shadow_offset)
{
    const char* who = "rdx_punctual_light_hits";
    if (!g.initialized) return fail("rdx_punctual_light_hits: rdx_init has not been called");
    static_assert(sizeof(rdx_punctual_light) == sizeof(PunctualLight) && RDX_MAX_PATH_LIGHTS == MAX_PATH_LIGHTS && RDX_LIGHT_SPOT == LIGHT_SPOT, "light table record");
    // the first three are read, the others written
    const CallRange R[5] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true},
                            {materials, materials_offset, (size_t)n * sizeof(rdx_material_record), "material-record", 16, true},
                            {lights, light_offset, sizeof(PunctualLight), "light", 16, true},
                            {lit, lit_offset, (size_t)n * 4 * sizeof(float), "lit", 16, true}, {shadow, shadow_offset, (size_t)n * sizeof(rdx_ray), "shadow-ray", 16, false}};
    if (check_call_handles(who, R)) return -1;
    if (check_call_ranges(who, R, 3, n)) return -1;
    if (!n) return 0;
    return timed_launch(&rdx_trace_stats::ms_shade, {lit, shadow}, [&] {
        launch_punctual_light_hits(g.stream, at<const float4>(rays, rays_offset), at<const float4>(materials, materials_offset), n,
                                   at<const PunctualLight>(lights, light_offset), at<float4>(lit, lit_offset), at<float4>(shadow, shadow_offset)); });
}

// rdx_trace_paths_lights over the first light_count records of a caller's light table (include/rdx.h; punctual.hip): the checks, then
// trace_light_paths with k_punctual_shade.  The SceneProperties stays a row although its lights are not read, so that what
// rdx_trace_paths_lights refuses is refused here
extern "C" int rdx_trace_paths_punctual(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n,
                                        uint32_t max_depth, rdx_buffer lights, size_t lights_offset, uint32_t light_count,
                                        const rdx_shading_buffers* scene, rdx_buffer radiance, size_t radiance_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_trace_paths_punctual";
    if (!g.initialized) return fail("rdx_trace_paths_punctual: rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_paths_punctual: invalid TLAS handle");
    if (light_count > MAX_PATH_LIGHTS)
        return fail("rdx_trace_paths_punctual: light_count %u exceeds the %u records a path samples (RDX_MAX_PATH_LIGHTS)", light_count, MAX_PATH_LIGHTS);
    const CallRange R[5] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true},
                            {lights, lights_offset, (size_t)light_count * sizeof(PunctualLight), "light-table", 16, true},
                            {scene ? scene->scene : nullptr, 0, sizeof(SceneProperties), "scene (SceneProperties)", 4, false},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (max_depth > 62) return fail("rdx_trace_paths_punctual: depth %u exceeds the supported maximum of 62", max_depth);
    if (check_call_ranges(who, R, 4, n, {invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    const PunctualLight* table = at<const PunctualLight>(lights, lights_offset);      // a device address: read by the kernels of every call
    return trace_light_paths(who, tlas, rays, rays_offset, keys, keys_offset, n, max_depth, light_count, sc, radiance, radiance_offset, invalid_out,
                             [&](hipStream_t st, const AccelCache& ac, const LightPathStreams& io, uint32_t live, uint32_t d, bool sampleNext, uint32_t* cursor,
                                 uint32_t* invalid) {
                                 launch_punctual_shade(st, ac.insts, ac.slotOf, ac.s.nInst, sc, table, light_count, io, live, d, sampleNext, cursor, invalid); });
}

// One record of a caller's area light table on material records (area.hip).  As rdx_punctual_light_hits, plus the one key or the
// one float4 of randoms per ray that rdx_scatter_hits reads, by its rule: exactly one of the two
extern "C" int rdx_area_light_hits(rdx_buffer rays, size_t rays_offset, rdx_buffer materials, size_t materials_offset, uint32_t n, rdx_buffer lights,
                                   size_t light_offset, rdx_buffer keys, size_t keys_offset, uint32_t stream, rdx_buffer randoms, size_t randoms_offset,
                                   rdx_buffer lit, size_t lit_offset, rdx_buffer shadow, size_t shadow_offset)
{
    const char* who = "rdx_area_light_hits";
    if (!g.initialized) return fail("rdx_area_light_hits: rdx_init has not been called");
    static_assert(sizeof(rdx_area_light) == sizeof(AreaLight) && RDX_AREA_TRIANGLE == AREA_TRIANGLE && RDX_AREA_TWO_SIDED == AREA_TWO_SIDED, "area light table record");
    // the first five are read, the others written
    const CallRange R[7] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true},
                            {materials, materials_offset, (size_t)n * sizeof(rdx_material_record), "material-record", 16, true},
                            {lights, light_offset, sizeof(AreaLight), "area-light", 16, true},
                            {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, false}, {randoms, randoms_offset, (size_t)n * 4 * sizeof(float), "randoms", 16, false},
                            {lit, lit_offset, (size_t)n * 4 * sizeof(float), "lit", 16, true}, {shadow, shadow_offset, (size_t)n * sizeof(rdx_ray), "shadow-ray", 16, false}};
    if (check_call_handles(who, R)) return -1;
    if (!keys && !randoms) return fail("rdx_area_light_hits: neither keys nor randoms given: one of the two is required");
    if (keys && randoms) return fail("rdx_area_light_hits: both keys and randoms given: only one of the two is allowed");
    if (stream > 0xfffeu) return fail("rdx_area_light_hits: stream %u exceeds the supported maximum of 65534", stream);
    if (check_call_ranges(who, R, 5, n)) return -1;
    if (!n) return 0;
    return timed_launch(&rdx_trace_stats::ms_shade, {lit, shadow}, [&] {
        launch_area_light_hits(g.stream, at<const float4>(rays, rays_offset), at<const float4>(materials, materials_offset), n,
                               at<const AreaLight>(lights, light_offset), at<const uint4>(keys, keys_offset), stream, at<const float4>(randoms, randoms_offset),
                               at<float4>(lit, lit_offset), at<float4>(shadow, shadow_offset)); });
}

// rdx_trace_paths_punctual over two tables (include/rdx.h; area.hip): the checks, then trace_light_paths with k_area_shade over
// light_count punctual records followed by area_count area records.  A table whose count is 0 may be NULL: its row is optional then
extern "C" int rdx_trace_paths_area(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n,
                                    uint32_t max_depth, rdx_buffer lights, size_t lights_offset, uint32_t light_count, rdx_buffer area,
                                    size_t area_offset, uint32_t area_count, const rdx_shading_buffers* scene, rdx_buffer radiance,
                                    size_t radiance_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_trace_paths_area";
    if (!g.initialized) return fail("rdx_trace_paths_area: rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_paths_area: invalid TLAS handle");
    if (light_count > MAX_PATH_LIGHTS || area_count > MAX_PATH_LIGHTS || light_count + area_count > MAX_PATH_LIGHTS)
        return fail("rdx_trace_paths_area: light_count %u + area_count %u exceeds the %u records a path samples (RDX_MAX_PATH_LIGHTS)", light_count, area_count,
                    MAX_PATH_LIGHTS);
    const CallRange R[6] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true},
                            {lights, lights_offset, (size_t)light_count * sizeof(PunctualLight), "light-table", 16, light_count != 0},
                            {area, area_offset, (size_t)area_count * sizeof(AreaLight), "area-light-table", 16, area_count != 0},
                            {scene ? scene->scene : nullptr, 0, sizeof(SceneProperties), "scene (SceneProperties)", 4, false},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (max_depth > 62) return fail("rdx_trace_paths_area: depth %u exceeds the supported maximum of 62", max_depth);
    if (check_call_ranges(who, R, 5, n, {invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    // device addresses: read by the kernels of every call.  A table of no records is never read
    const PunctualLight* table = light_count ? at<const PunctualLight>(lights, lights_offset) : nullptr;
    const AreaLight* areaTable = area_count ? at<const AreaLight>(area, area_offset) : nullptr;
    return trace_light_paths(who, tlas, rays, rays_offset, keys, keys_offset, n, max_depth, light_count + area_count, sc, radiance, radiance_offset, invalid_out,
                             [&](hipStream_t st, const AccelCache& ac, const LightPathStreams& io, uint32_t live, uint32_t d, bool sampleNext, uint32_t* cursor,
                                 uint32_t* invalid) {
                                 launch_area_shade(st, ac.insts, ac.slotOf, ac.s.nInst, sc, table, light_count, areaTable, area_count, io, live, d, sampleNext, cursor,
                                                   invalid); });
}

// ---- the environment: a lat-long image and the sampling table rdx_env_build derives from it (include/rdx.h; env.h, env.hip) ----
namespace {
int env_size_refused(const char* who, uint32_t width, uint32_t height)
{
    if (env_table_size(width, height)) return 0;
    return fail("%s: an environment of %u x %u texels is outside the supported 1 .. %u x 1 .. %u", who, width, height, ENV_MAX_WIDTH, ENV_MAX_HEIGHT);
}
size_t env_image_bytes(uint32_t width, uint32_t height) { return (size_t)width * height * 4 * sizeof(float); }
EnvView env_view(rdx_buffer image, size_t image_offset, rdx_buffer table, size_t table_offset, uint32_t width, uint32_t height)
{
    return EnvView{at<const float4>(image, image_offset), at<const char>(table, table_offset), width, height};
}
} // namespace

extern "C" size_t rdx_env_table_size(uint32_t width, uint32_t height) { return env_table_size(width, height); }

// The header and rowCos are computed here (cosines in double) and uploaded, the padding of the parts is zeroed, and the three
// kernels follow in stream order: nothing comes back to the host before the table is complete
extern "C" int rdx_env_build(rdx_buffer image, size_t image_offset, uint32_t width, uint32_t height, rdx_buffer table, size_t table_offset)
{
    const char* who = "rdx_env_build";
    if (!g.initialized) return fail("rdx_env_build: rdx_init has not been called");
    if (env_size_refused(who, width, height)) return -1;
    const CallRange R[2] = {{image, image_offset, env_image_bytes(width, height), "environment-image", 16, true},
                            {table, table_offset, env_table_size(width, height), "environment-table", 16, true}};
    if (check_call_handles(who, R)) return -1;
    if (check_call_ranges(who, R, 1, 1)) return -1;
    std::vector<char> head(env_c_offset(height), 0);
    EnvHeader hd{};
    hd.magic = ENV_MAGIC; hd.version = ENV_VERSION; hd.width = width; hd.height = height;
    const double pi = 3.14159265358979323846;
    hd.twoPiOverW = (float)(2.0 * pi / (double)width);
    hd.wOverTwoPi = (float)((double)width / (2.0 * pi));
    std::memcpy(head.data(), &hd, sizeof hd);
    float* rowCos = reinterpret_cast<float*>(head.data() + env_rowcos_offset());
    for (uint32_t y = 0; y <= height; ++y) rowCos[y] = (float)std::cos(pi * (double)y / (double)height);
    rowCos[0] = 1.0f; rowCos[height] = -1.0f;
    char* dTable = at<char>(table, table_offset);
    const size_t cEnd = env_c_offset(height) + (size_t)width * height * sizeof(uint32_t), mEnd = env_m_offset(width, height) + (size_t)height * sizeof(uint64_t);
    return timed_launch(&rdx_trace_stats::ms_shade, {table}, [&] {
        HIP_IGN(hipMemcpyAsync(dTable, head.data(), head.size(), hipMemcpyHostToDevice, g.stream));
        if (env_m_offset(width, height) > cEnd) HIP_IGN(hipMemsetAsync(dTable + cEnd, 0, env_m_offset(width, height) - cEnd, g.stream));
        if (env_table_size(width, height) > mEnd) HIP_IGN(hipMemsetAsync(dTable + mEnd, 0, env_table_size(width, height) - mEnd, g.stream));
        launch_env_build(g.stream, at<const float4>(image, image_offset), dTable, width, height); });
}

// rdx_area_light_hits with the environment in the place of the one record (env.hip): light_hits around env_emit
extern "C" int rdx_env_light_hits(rdx_buffer rays, size_t rays_offset, rdx_buffer materials, size_t materials_offset, uint32_t n, rdx_buffer image,
                                  size_t image_offset, rdx_buffer table, size_t table_offset, uint32_t width, uint32_t height, rdx_buffer keys,
                                  size_t keys_offset, uint32_t stream, rdx_buffer randoms, size_t randoms_offset, rdx_buffer lit, size_t lit_offset,
                                  rdx_buffer shadow, size_t shadow_offset)
{
    const char* who = "rdx_env_light_hits";
    if (!g.initialized) return fail("rdx_env_light_hits: rdx_init has not been called");
    if (env_size_refused(who, width, height)) return -1;
    // the first six are read, the others written
    const CallRange R[8] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true},
                            {materials, materials_offset, (size_t)n * sizeof(rdx_material_record), "material-record", 16, true},
                            {image, image_offset, env_image_bytes(width, height), "environment-image", 16, true},
                            {table, table_offset, env_table_size(width, height), "environment-table", 16, true},
                            {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, false}, {randoms, randoms_offset, (size_t)n * 4 * sizeof(float), "randoms", 16, false},
                            {lit, lit_offset, (size_t)n * 4 * sizeof(float), "lit", 16, true}, {shadow, shadow_offset, (size_t)n * sizeof(rdx_ray), "shadow-ray", 16, false}};
    if (check_call_handles(who, R)) return -1;
    if (!keys && !randoms) return fail("rdx_env_light_hits: neither keys nor randoms given: one of the two is required");
    if (keys && randoms) return fail("rdx_env_light_hits: both keys and randoms given: only one of the two is allowed");
    if (stream > 0xfffeu) return fail("rdx_env_light_hits: stream %u exceeds the supported maximum of 65534", stream);
    if (check_call_ranges(who, R, 6, n)) return -1;
    if (!n) return 0;
    return timed_launch(&rdx_trace_stats::ms_shade, {lit, shadow}, [&] {
        launch_env_light_hits(g.stream, at<const float4>(rays, rays_offset), at<const float4>(materials, materials_offset), n,
                              env_view(image, image_offset, table, table_offset, width, height), at<const uint4>(keys, keys_offset), stream,
                              at<const float4>(randoms, randoms_offset), at<float4>(lit, lit_offset), at<float4>(shadow, shadow_offset)); });
}

// the texel the environment shows along each ray's direction (env.hip): env_lookup per ray
extern "C" int rdx_env_lookup(rdx_buffer rays, size_t rays_offset, uint32_t n, rdx_buffer image, size_t image_offset, rdx_buffer table, size_t table_offset,
                              uint32_t width, uint32_t height, rdx_buffer radiance, size_t radiance_offset)
{
    const char* who = "rdx_env_lookup";
    if (!g.initialized) return fail("rdx_env_lookup: rdx_init has not been called");
    if (env_size_refused(who, width, height)) return -1;
    const CallRange R[4] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true},
                            {image, image_offset, env_image_bytes(width, height), "environment-image", 16, true},
                            {table, table_offset, env_table_size(width, height), "environment-table", 16, true},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true}};
    if (check_call_handles(who, R)) return -1;
    if (check_call_ranges(who, R, 3, n)) return -1;
    if (!n) return 0;
    return timed_launch(&rdx_trace_stats::ms_shade, {radiance}, [&] {
        launch_env_lookup(g.stream, at<const float4>(rays, rays_offset), n, env_view(image, image_offset, table, table_offset, width, height),
                          at<float4>(radiance, radiance_offset)); });
}

// rdx_trace_paths_area with the environment as one more record after the two tables (include/rdx.h; env.hip): the checks, then
// trace_light_paths with k_env_shade over light_count + area_count + 1 records
extern "C" int rdx_trace_paths_env(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n, uint32_t max_depth,
                                   rdx_buffer lights, size_t lights_offset, uint32_t light_count, rdx_buffer area, size_t area_offset, uint32_t area_count,
                                   rdx_buffer image, size_t image_offset, rdx_buffer table, size_t table_offset, uint32_t width, uint32_t height,
                                   const rdx_shading_buffers* scene, rdx_buffer radiance, size_t radiance_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_trace_paths_env";
    if (!g.initialized) return fail("rdx_trace_paths_env: rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_paths_env: invalid TLAS handle");
    if (light_count >= MAX_PATH_LIGHTS || area_count >= MAX_PATH_LIGHTS || light_count + area_count + 1 > MAX_PATH_LIGHTS)
        return fail("rdx_trace_paths_env: light_count %u + area_count %u + the environment exceeds the %u records a path samples (RDX_MAX_PATH_LIGHTS)", light_count,
                    area_count, MAX_PATH_LIGHTS);
    if (env_size_refused(who, width, height)) return -1;
    const CallRange R[8] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true},
                            {lights, lights_offset, (size_t)light_count * sizeof(PunctualLight), "light-table", 16, light_count != 0},
                            {area, area_offset, (size_t)area_count * sizeof(AreaLight), "area-light-table", 16, area_count != 0},
                            {image, image_offset, env_image_bytes(width, height), "environment-image", 16, true},
                            {table, table_offset, env_table_size(width, height), "environment-table", 16, true},
                            {scene ? scene->scene : nullptr, 0, sizeof(SceneProperties), "scene (SceneProperties)", 4, false},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (max_depth > 62) return fail("rdx_trace_paths_env: depth %u exceeds the supported maximum of 62", max_depth);
    if (check_call_ranges(who, R, 7, n, {invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    // device addresses: read by the kernels of every call.  A table of no records is never read
    const PunctualLight* lightTable = light_count ? at<const PunctualLight>(lights, lights_offset) : nullptr;
    const AreaLight* areaTable = area_count ? at<const AreaLight>(area, area_offset) : nullptr;
    const EnvView env = env_view(image, image_offset, table, table_offset, width, height);
    return trace_light_paths(who, tlas, rays, rays_offset, keys, keys_offset, n, max_depth, light_count + area_count + 1, sc, radiance, radiance_offset, invalid_out,
                             [&](hipStream_t st, const AccelCache& ac, const LightPathStreams& io, uint32_t live, uint32_t d, bool sampleNext, uint32_t* cursor,
                                 uint32_t* invalid) {
                                 launch_env_shade(st, ac.insts, ac.slotOf, ac.s.nInst, sc, lightTable, light_count, areaTable, area_count, env, io, live, d, sampleNext,
                                                  cursor, invalid); });
}

// The weight of the scatter sample against the environment's for n directions (include/rdx.h; env_mis.hip).  As rdx_env_light_hits:
// no TLAS and no scene streams, so the checks are those of the ranges alone.  rays, materials, keys and randoms hold nrecords rows,
// dirs, src and out n
extern "C" int rdx_env_mis_weights(rdx_buffer rays, size_t rays_offset, rdx_buffer materials, size_t materials_offset, rdx_buffer dirs, size_t dirs_offset,
                                   uint32_t n, rdx_buffer src, size_t src_offset, uint32_t nrecords, rdx_buffer keys, size_t keys_offset, rdx_buffer randoms,
                                   size_t randoms_offset, rdx_buffer image, size_t image_offset, rdx_buffer table, size_t table_offset, uint32_t width,
                                   uint32_t height, rdx_buffer out, size_t out_offset)
{
    const char* who = "rdx_env_mis_weights";
    if (!g.initialized) return fail("rdx_env_mis_weights: rdx_init has not been called");
    if (env_size_refused(who, width, height)) return -1;
    static_assert(sizeof(rdx_env_mis_weight) == 16 && RDX_LOBE_NONE == LOBE_NONE && RDX_LOBE_TRANSMISSION == LOBE_TRANSMISSION, "weight record");
    // the first eight are read, the last written
    const CallRange R[9] = {{rays, rays_offset, (size_t)nrecords * sizeof(rdx_ray), "ray", 16, true},
                            {materials, materials_offset, (size_t)nrecords * sizeof(rdx_material_record), "material-record", 16, true},
                            {dirs, dirs_offset, (size_t)n * sizeof(rdx_ray), "direction", 16, true},
                            {src, src_offset, (size_t)n * sizeof(uint32_t), "src", 4, false},
                            {image, image_offset, env_image_bytes(width, height), "environment-image", 16, true},
                            {table, table_offset, env_table_size(width, height), "environment-table", 16, true},
                            {keys, keys_offset, (size_t)nrecords * sizeof(rdx_shade_key), "key", 16, false},
                            {randoms, randoms_offset, (size_t)nrecords * 4 * sizeof(float), "randoms", 16, false},
                            {out, out_offset, (size_t)n * sizeof(rdx_env_mis_weight), "weight", 16, true}};
    if (check_call_handles(who, R)) return -1;
    if (keys && randoms) return fail("rdx_env_mis_weights: both keys and randoms given: at most one of the two is allowed");
    if (!src && nrecords != n) return fail("rdx_env_mis_weights: without src direction k belongs to record k: nrecords %u must equal n %u", nrecords, n);
    if (check_call_ranges(who, R, 8, n)) return -1;
    if (!n) return 0;
    return timed_launch(&rdx_trace_stats::ms_shade, {out}, [&] {
        launch_env_mis_weights(g.stream, at<const float4>(rays, rays_offset), at<const float4>(materials, materials_offset), at<const float4>(dirs, dirs_offset), n,
                               at<const uint32_t>(src, src_offset), nrecords, at<const uint4>(keys, keys_offset), at<const float4>(randoms, randoms_offset),
                               env_view(image, image_offset, table, table_offset, width, height), at<uint4>(out, out_offset)); });
}

// rdx_trace_paths_env with the environment and the scatter sample weighted against each other (include/rdx.h; env_mis.hip): the
// checks of rdx_trace_paths_env, then trace_light_paths with k_env_mis_shade and k_env_mis_fold
extern "C" int rdx_trace_paths_env_mis(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer keys, size_t keys_offset, uint32_t n, uint32_t max_depth,
                                       rdx_buffer lights, size_t lights_offset, uint32_t light_count, rdx_buffer area, size_t area_offset, uint32_t area_count,
                                       rdx_buffer image, size_t image_offset, rdx_buffer table, size_t table_offset, uint32_t width, uint32_t height,
                                       const rdx_shading_buffers* scene, rdx_buffer radiance, size_t radiance_offset, uint32_t* invalid_out)
{
    const char* who = "rdx_trace_paths_env_mis";
    if (!g.initialized) return fail("rdx_trace_paths_env_mis: rdx_init has not been called");
    if (!tlas || !known_buffer(tlas)) return fail("rdx_trace_paths_env_mis: invalid TLAS handle");
    if (light_count >= MAX_PATH_LIGHTS || area_count >= MAX_PATH_LIGHTS || light_count + area_count + 1 > MAX_PATH_LIGHTS)
        return fail("rdx_trace_paths_env_mis: light_count %u + area_count %u + the environment exceeds the %u records a path samples (RDX_MAX_PATH_LIGHTS)",
                    light_count, area_count, MAX_PATH_LIGHTS);
    if (env_size_refused(who, width, height)) return -1;
    const CallRange R[8] = {{rays, rays_offset, (size_t)n * sizeof(rdx_ray), "ray", 16, true}, {keys, keys_offset, (size_t)n * sizeof(rdx_shade_key), "key", 16, true},
                            {lights, lights_offset, (size_t)light_count * sizeof(PunctualLight), "light-table", 16, light_count != 0},
                            {area, area_offset, (size_t)area_count * sizeof(AreaLight), "area-light-table", 16, area_count != 0},
                            {image, image_offset, env_image_bytes(width, height), "environment-image", 16, true},
                            {table, table_offset, env_table_size(width, height), "environment-table", 16, true},
                            {scene ? scene->scene : nullptr, 0, sizeof(SceneProperties), "scene (SceneProperties)", 4, false},
                            {radiance, radiance_offset, (size_t)n * sizeof(float4), "radiance", 16, true}};
    uint32_t samplerBits = 0;
    if (check_call_handles(who, R) || check_shading_handles(who, scene, samplerBits)) return -1;
    if (max_depth > 62) return fail("rdx_trace_paths_env_mis: depth %u exceeds the supported maximum of 62", max_depth);
    if (check_call_ranges(who, R, 7, n, {invalid_out}, shading_aligned(scene))) return -1;
    if (!n) return 0;
    ShadeScene sc;
    if (shade_scene(who, scene, samplerBits, sc) || derive_accel(tlas)) return -1;
    const PunctualLight* lightTable = light_count ? at<const PunctualLight>(lights, lights_offset) : nullptr;
    const AreaLight* areaTable = area_count ? at<const AreaLight>(area, area_offset) : nullptr;
    const EnvView env = env_view(image, image_offset, table, table_offset, width, height);
    return trace_light_paths(who, tlas, rays, rays_offset, keys, keys_offset, n, max_depth, light_count + area_count + 1, sc, radiance, radiance_offset, invalid_out,
                             [&](hipStream_t st, const AccelCache& ac, const LightPathStreams& io, uint32_t live, uint32_t d, bool sampleNext, uint32_t* cursor,
                                 uint32_t* invalid) {
                                 launch_env_mis_shade(st, ac.insts, ac.slotOf, ac.s.nInst, sc, lightTable, light_count, areaTable, area_count, env, io, live, d,
                                                      sampleNext, cursor, invalid); },
                             launch_env_mis_fold);
}

// ---- the edge-avoiding a-trous filter over a frame's colours (denoise.hip) ---------------------------------------------
namespace {
uint32_t g_denoiseTiled = 3;        // rdx_debug_denoise_tiled: steps 1 and 2 from the LDS tile, the faster form of both
}

extern "C" size_t rdx_denoise_work_size(uint32_t width, uint32_t height) { return denoise_work_size(width, height); }

// Test and measurement seam: bit j set = pass j (j < 2: steps 1 and 2) of every later rdx_denoise takes its taps from an LDS tile,
// clear = straight from memory.  Both forms give the same bits; the default, 3, is what was measured faster
extern "C" void rdx_debug_denoise_tiled(uint32_t mask) { g_denoiseTiled = mask & 3u; }

extern "C" int rdx_denoise(rdx_buffer color, size_t color_offset, rdx_buffer materials, size_t materials_offset, rdx_buffer surfaces, size_t surfaces_offset,
                           uint32_t width, uint32_t height, const rdx_denoise_settings* settings, rdx_buffer work, size_t work_offset, rdx_buffer out,
                           size_t out_offset, rdx_buffer image, size_t image_offset)
{
    const char* who = "rdx_denoise";
    if (!g.initialized) return fail("rdx_denoise: rdx_init has not been called");
    static_assert(sizeof(rdx_denoise_settings) == 32 && sizeof(rdx_material_record) == 64 && sizeof(rdx_surface) == 64, "the records of rdx_denoise");
    const bool empty = !width || !height;
    const size_t npix = empty ? 0 : (size_t)width * height;
    // a size outside the limits is refused below, before the table is consulted: until then the byte counts only have to exist
    const size_t rows = npix <= DENOISE_MAX_PIXELS ? npix : 0;
    const CallRange R[6] = {{color, color_offset, rows * sizeof(float4), "colour", 16, true},
                            {materials, materials_offset, rows * sizeof(rdx_material_record), "material-record", 16, true},
                            {surfaces, surfaces_offset, rows * sizeof(rdx_surface), "surface-record", 16, true},
                            {work, work_offset, empty ? 0 : denoise_work_size(width, height), "work", 16, true},
                            {out, out_offset, rows * sizeof(float4), "output", 16, true}, {image, image_offset, rows * 4, "image", 4, false}};
    if (check_call_handles(who, R)) return -1;
    if (!settings) return fail("rdx_denoise: no settings");
    if (settings->passes > DENOISE_MAX_PASSES) return fail("rdx_denoise: %u passes exceed the supported maximum of %u", settings->passes, DENOISE_MAX_PASSES);
    if (settings->normal_squarings > DENOISE_MAX_SQUARINGS)
        return fail("rdx_denoise: normal_squarings %u exceeds the supported maximum of %u", settings->normal_squarings, DENOISE_MAX_SQUARINGS);
    if (!(settings->sigma_position >= 0.0f && settings->sigma_position < HUGE_VALF))
        return fail("rdx_denoise: sigma_position must be 0 (the term is off) or finite and positive, not %g", (double)settings->sigma_position);
    if (!(settings->sigma_colour >= 0.0f && settings->sigma_colour < HUGE_VALF))
        return fail("rdx_denoise: sigma_colour must be 0 (the term is off) or finite and positive, not %g", (double)settings->sigma_colour);
    if (settings->flags & ~(RDX_DENOISE_DEMODULATE | RDX_DENOISE_DEBUG))
        return fail("rdx_denoise: unknown flags 0x%x (bit 0 = demodulate, bit 1 = debug)", settings->flags);
    if (settings->_0[0] | settings->_0[1] | settings->_0[2]) return fail("rdx_denoise: the padding of the settings must be 0");
    if (!empty && !denoise_work_size(width, height))
        return fail("rdx_denoise: an image of %u x %u pixels is outside the supported 1 .. %u x 1 .. %u and 2^26 pixels", width, height, DENOISE_MAX_DIM,
                    DENOISE_MAX_DIM);
    if (check_call_ranges(who, R, 3, (uint32_t)npix)) return -1;
    if (empty) return 0;
    const DenoiseArgs a{width, height, settings->passes, settings->normal_squarings, settings->flags, settings->sigma_position, settings->sigma_colour, g_denoiseTiled};
    return timed_launch(&rdx_trace_stats::ms_accumulate, {work, out, image}, [&] {
        launch_denoise(g.stream, a, at<const float4>(color, color_offset), at<const float4>(materials, materials_offset), at<const float4>(surfaces, surfaces_offset),
                       at<float4>(work, work_offset), at<float4>(out, out_offset), at<uchar4>(image, image_offset)); });
}

// ---- temporal accumulation: a frame's history reprojected through the previous view (temporal.hip) -------------------
extern "C" size_t rdx_temporal_history_size(uint32_t width, uint32_t height) { return temporal_history_size(width, height); }

extern "C" int rdx_camera_view(rdx_buffer camera, rdx_buffer view, size_t view_offset)
{
    const char* who = "rdx_camera_view";
    if (!g.initialized) return fail("rdx_camera_view: rdx_init has not been called");
    static_assert(sizeof(rdx_view) == 64, "four float4 per view");
    const CallRange R[2] = {{camera, 0, sizeof(PhysicalCamera), "camera", 4, true}, {view, view_offset, sizeof(rdx_view), "view", 16, true}};
    if (check_call_handles(who, R)) return -1;
    if (camera->size < sizeof(PhysicalCamera))
        return fail("rdx_camera_view: the camera buffer (%zu bytes) does not hold a PhysicalCamera (%zu bytes)", camera->size, sizeof(PhysicalCamera));
    if (check_call_ranges(who, R, 1, 1)) return -1;
    return timed_launch(&rdx_trace_stats::ms_generate, {view}, [&] {
        launch_camera_view(g.stream, at<const PhysicalCamera>(camera), at<float4>(view, view_offset)); });
}

extern "C" int rdx_temporal_accumulate(rdx_buffer color, size_t color_offset, rdx_buffer materials, size_t materials_offset, rdx_buffer surfaces,
                                       size_t surfaces_offset, rdx_buffer previous_positions, size_t previous_positions_offset, rdx_buffer view,
                                       size_t view_offset, rdx_buffer previous_view, size_t previous_view_offset, uint32_t width, uint32_t height,
                                       const rdx_temporal_settings* settings, rdx_buffer history_in, size_t history_in_offset, rdx_buffer history_out,
                                       size_t history_out_offset, rdx_buffer image, size_t image_offset)
{
    const char* who = "rdx_temporal_accumulate";
    if (!g.initialized) return fail("rdx_temporal_accumulate: rdx_init has not been called");
    static_assert(sizeof(rdx_temporal_settings) == 32 && sizeof(rdx_view) == 64, "the records of rdx_temporal_accumulate");
    const bool empty = !width || !height;
    const size_t npix = empty ? 0 : (size_t)width * height;
    // a size outside the limits is refused below, before the table is consulted: until then the byte counts only have to exist
    const size_t rows = npix <= TEMPORAL_MAX_PIXELS ? npix : 0;
    const size_t history = empty ? 0 : temporal_history_size(width, height);
    const CallRange R[9] = {{color, color_offset, rows * sizeof(float4), "colour", 16, true},
                            {materials, materials_offset, rows * sizeof(rdx_material_record), "material-record", 16, true},
                            {surfaces, surfaces_offset, rows * sizeof(rdx_surface), "surface-record", 16, true},
                            {previous_positions, previous_positions_offset, rows * sizeof(float4), "previous-position", 16, false},
                            {view, view_offset, empty ? 0 : sizeof(rdx_view), "view", 16, true},
                            {previous_view, previous_view_offset, empty ? 0 : sizeof(rdx_view), "previous-view", 16, false},
                            {history_in, history_in_offset, history, "history-in", 16, false},
                            {history_out, history_out_offset, history, "history-out", 16, true},
                            {image, image_offset, rows * 4, "image", 4, false}};
    if (check_call_handles(who, R)) return -1;
    if (!settings) return fail("rdx_temporal_accumulate: no settings");
    const rdx_temporal_settings& s = *settings;
    if (s.max_history < 1u || s.max_history > TEMPORAL_MAX_HISTORY)
        return fail("rdx_temporal_accumulate: max_history %u is outside 1 .. %u", s.max_history, TEMPORAL_MAX_HISTORY);
    if (!(s.alpha_min >= 0.0f && s.alpha_min <= 1.0f)) return fail("rdx_temporal_accumulate: alpha_min must lie in [0, 1], not %g", (double)s.alpha_min);
    if (!(s.alpha_moments_min >= 0.0f && s.alpha_moments_min <= 1.0f))
        return fail("rdx_temporal_accumulate: alpha_moments_min must lie in [0, 1], not %g", (double)s.alpha_moments_min);
    if (!(std::fabs(s.normal_cos_min) < HUGE_VALF)) return fail("rdx_temporal_accumulate: normal_cos_min must be finite, not %g", (double)s.normal_cos_min);
    if (!(s.position_tolerance >= 0.0f && s.position_tolerance < HUGE_VALF))
        return fail("rdx_temporal_accumulate: position_tolerance must be 0 (the term is off) or finite and positive, not %g", (double)s.position_tolerance);
    if (s.variance_min_history > TEMPORAL_MAX_VARIANCE_HISTORY)
        return fail("rdx_temporal_accumulate: variance_min_history %u exceeds the supported maximum of %u", s.variance_min_history, TEMPORAL_MAX_VARIANCE_HISTORY);
    if (s.flags & ~RDX_TEMPORAL_DEBUG) return fail("rdx_temporal_accumulate: unknown flags 0x%x (bit 0 = debug)", s.flags);
    if (s._0) return fail("rdx_temporal_accumulate: the padding of the settings must be 0");
    if (!empty && !history)
        return fail("rdx_temporal_accumulate: an image of %u x %u pixels is outside the supported 1 .. %u x 1 .. %u and 2^26 pixels", width, height,
                    TEMPORAL_MAX_DIM, TEMPORAL_MAX_DIM);
    if (check_call_ranges(who, R, 7, (uint32_t)npix)) return -1;
    if (empty) return 0;
    TemporalArgs a{width, height, s.max_history, s.variance_min_history, s.flags & TEMPORAL_DEBUG, s.alpha_min, s.alpha_moments_min, s.normal_cos_min,
                   s.position_tolerance};
    if (s.position_tolerance != 0.0f) a.flags |= TEMPORAL_POSITION;
    const float4* v = at<const float4>(view, view_offset);
    return timed_launch(&rdx_trace_stats::ms_accumulate, {history_out, image}, [&] {
        launch_temporal_accumulate(g.stream, a, at<const float4>(color, color_offset), at<const float4>(materials, materials_offset),
                                   at<const float4>(surfaces, surfaces_offset), at<const float4>(previous_positions, previous_positions_offset), v,
                                   previous_view ? at<const float4>(previous_view, previous_view_offset) : v, at<const float4>(history_in, history_in_offset),
                                   at<float4>(history_out, history_out_offset), at<uchar4>(image, image_offset)); });
}

// ---- the variance-guided a-trous filter of SVGF over a history's colours and variance (svgf.hip) -----------------------
namespace {
uint32_t g_svgfTiled = 3;           // rdx_debug_svgf_tiled: which of steps 1 and 2 take the LDS tile
}

extern "C" size_t rdx_svgf_work_size(uint32_t width, uint32_t height) { return svgf_work_size(width, height); }

// Test and measurement seam: bit j set = pass j (j < 2: steps 1 and 2) of every later rdx_svgf_filter takes its taps from an LDS
// tile, clear = straight from memory.  Both forms give the same bits
extern "C" void rdx_debug_svgf_tiled(uint32_t mask) { g_svgfTiled = mask & 3u; }

extern "C" int rdx_svgf_filter(rdx_buffer color, size_t color_offset, rdx_buffer moments, size_t moments_offset, rdx_buffer materials, size_t materials_offset,
                               rdx_buffer surfaces, size_t surfaces_offset, uint32_t width, uint32_t height, const rdx_svgf_settings* settings, rdx_buffer work,
                               size_t work_offset, rdx_buffer out, size_t out_offset, rdx_buffer variance_out, size_t variance_out_offset, rdx_buffer feedback,
                               size_t feedback_offset, rdx_buffer image, size_t image_offset)
{
    const char* who = "rdx_svgf_filter";
    if (!g.initialized) return fail("rdx_svgf_filter: rdx_init has not been called");
    static_assert(sizeof(rdx_svgf_settings) == 32 && sizeof(rdx_material_record) == 64 && sizeof(rdx_surface) == 64, "the records of rdx_svgf_filter");
    const bool empty = !width || !height;
    const size_t npix = empty ? 0 : (size_t)width * height;
    // a size outside the limits is refused below, before the table is consulted: until then the byte counts only have to exist
    const size_t rows = npix <= DENOISE_MAX_PIXELS ? npix : 0;
    const CallRange R[9] = {{color, color_offset, rows * sizeof(float4), "colour", 16, true},
                            {moments, moments_offset, rows * sizeof(float4), "moments", 16, true},
                            {materials, materials_offset, rows * sizeof(rdx_material_record), "material-record", 16, true},
                            {surfaces, surfaces_offset, rows * sizeof(rdx_surface), "surface-record", 16, true},
                            {work, work_offset, empty ? 0 : svgf_work_size(width, height), "work", 16, true},
                            {out, out_offset, rows * sizeof(float4), "output", 16, true},
                            {variance_out, variance_out_offset, rows * sizeof(float), "variance", 4, false},
                            {feedback, feedback_offset, rows * sizeof(float4), "feedback", 16, false},
                            {image, image_offset, rows * 4, "image", 4, false}};
    if (check_call_handles(who, R)) return -1;
    if (!settings) return fail("rdx_svgf_filter: no settings");
    const rdx_svgf_settings& s = *settings;
    if (s.passes > DENOISE_MAX_PASSES) return fail("rdx_svgf_filter: %u passes exceed the supported maximum of %u", s.passes, DENOISE_MAX_PASSES);
    if (s.normal_squarings > DENOISE_MAX_SQUARINGS)
        return fail("rdx_svgf_filter: normal_squarings %u exceeds the supported maximum of %u", s.normal_squarings, DENOISE_MAX_SQUARINGS);
    if (!(s.sigma_position >= 0.0f && s.sigma_position < HUGE_VALF))
        return fail("rdx_svgf_filter: sigma_position must be 0 (the term is off) or finite and positive, not %g", (double)s.sigma_position);
    if (!(s.sigma_luminance >= 0.0f && s.sigma_luminance < HUGE_VALF))
        return fail("rdx_svgf_filter: sigma_luminance must be 0 (the term is off) or finite and positive, not %g", (double)s.sigma_luminance);
    if (!(s.epsilon > 0.0f && s.epsilon < HUGE_VALF)) return fail("rdx_svgf_filter: epsilon must be finite and positive, not %g", (double)s.epsilon);
    if (s.feedback_pass > s.passes) return fail("rdx_svgf_filter: feedback_pass %u exceeds the %u passes", s.feedback_pass, s.passes);
    if (feedback && !s.feedback_pass) return fail("rdx_svgf_filter: a feedback buffer was given, but feedback_pass is 0");
    if (!feedback && s.feedback_pass) return fail("rdx_svgf_filter: feedback_pass is %u, but no feedback buffer was given", s.feedback_pass);
    if (s.flags & ~(RDX_DENOISE_DEMODULATE | RDX_DENOISE_DEBUG))
        return fail("rdx_svgf_filter: unknown flags 0x%x (bit 0 = demodulate, bit 1 = debug)", s.flags);
    if (s._0) return fail("rdx_svgf_filter: the padding of the settings must be 0");
    if (!empty && !svgf_work_size(width, height))
        return fail("rdx_svgf_filter: an image of %u x %u pixels is outside the supported 1 .. %u x 1 .. %u and 2^26 pixels", width, height, DENOISE_MAX_DIM,
                    DENOISE_MAX_DIM);
    if (check_call_ranges(who, R, 4, (uint32_t)npix)) return -1;
    if (empty) return 0;
    const SvgfArgs a{width, height, s.passes, s.normal_squarings, s.flags, s.sigma_position, s.sigma_luminance, s.epsilon, s.feedback_pass, g_svgfTiled};
    return timed_launch(&rdx_trace_stats::ms_accumulate, {work, out, variance_out, feedback, image}, [&] {
        launch_svgf_filter(g.stream, a, at<const float4>(color, color_offset), at<const float4>(moments, moments_offset),
                           at<const float4>(materials, materials_offset), at<const float4>(surfaces, surfaces_offset), at<float4>(work, work_offset),
                           at<float4>(out, out_offset), at<float>(variance_out, variance_out_offset), at<float4>(feedback, feedback_offset),
                           at<uchar4>(image, image_offset)); });
}

extern "C" int rdx_material_batch(const rdx_hit* hits, const float* dirs, const uint32_t* pixels, const uint32_t* frames,
                                  const int32_t* depths, uint32_t n, rdx_payload* out)
{
    if (!g.initialized) return fail("rdx_init has not been called");
    SceneArgs sc;
    if (scene_args(sc)) return -1;
    DevArray<rdx_hit> dH; DevArray<float> dD; DevArray<uint32_t> dP, dF; DevArray<int32_t> dDep; DevArray<rdx_payload> dO;
    HIP_OK(dH.upload(hits, n)); HIP_OK(dD.upload(dirs, 3 * (size_t)n)); HIP_OK(dP.upload(pixels, n));
    HIP_OK(dF.upload(frames, n)); HIP_OK(dDep.upload(depths, n)); HIP_OK(dO.alloc(n));
    launch_material_batch(g.stream, sc, dH.p, dD.p, dP.p, dF.p, dDep.p, n, dO.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    if (n) HIP_OK(hipMemcpy(out, dO.p, (size_t)n * sizeof(rdx_payload), hipMemcpyDeviceToHost));
    return 0;
}

extern "C" int rdx_generate_batch(const uint32_t* pixels, const uint32_t* rnd, uint32_t n, float* o, float* d)
{
    if (!g.initialized) return fail("rdx_init has not been called");
    if (!g.slots[3] || !known_buffer(g.slots[3])) return fail("descriptor slot 3 (camera) is not a buffer");
    PhysicalCamera cam;
    HIP_OK(hipMemcpy(&cam, static_cast<rdx_buffer_s*>(g.slots[3])->dptr, sizeof cam, hipMemcpyDeviceToHost));
    CameraArgs C;
    if (camera_args(cam, C)) return -1;
    DevArray<uint32_t> dP, dR; DevArray<float> dO, dD;
    HIP_OK(dP.upload(pixels, n)); HIP_OK(dR.upload(rnd, 3 * (size_t)n)); HIP_OK(dO.alloc(3 * (size_t)n)); HIP_OK(dD.alloc(3 * (size_t)n));
    launch_generate_batch(g.stream, C, dP.p, dR.p, n, dO.p, dD.p);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    if (n) { HIP_OK(hipMemcpy(o, dO.p, 12 * (size_t)n, hipMemcpyDeviceToHost)); HIP_OK(hipMemcpy(d, dD.p, 12 * (size_t)n, hipMemcpyDeviceToHost)); }
    return 0;
}

extern "C" int rdx_pcg3d_batch(const uint32_t* in3, float* out3, uint32_t n)
{
    if (!g.initialized) return fail("rdx_init has not been called");
    DevArray<uint32_t> dI; DevArray<float> dO;
    HIP_OK(dI.upload(in3, 3 * (size_t)n)); HIP_OK(dO.alloc(3 * (size_t)n));
    launch_pcg3d_batch(g.stream, dI.p, dO.p, n);
    HIP_OK(hipGetLastError());
    HIP_OK(hipStreamSynchronize(g.stream));
    if (n) HIP_OK(hipMemcpy(out3, dO.p, 12 * (size_t)n, hipMemcpyDeviceToHost));
    return 0;
}

static int export_layout(const AccelLayout& L, rdx_accel_scalars* scalars, void* const* arrays, size_t* bytes);

extern "C" int rdx_debug_accel_layout(const void* blob, size_t size, int quad, int cull, rdx_accel_scalars* scalars,
                                      void* const* arrays, size_t* bytes)
{
    if (!blob) return fail("rdx_debug_accel_layout: no blob");
    if (arrays && !bytes) return fail("rdx_debug_accel_layout: arrays need their capacities in bytes[]");
    AccelLayout L;
    std::string err;
    if (derive_accel_layout(blob, size, AccelOptions{quad, cull}, L, err)) return fail_str(err);
    return export_layout(L, scalars, arrays, bytes);
}

// blobs[0] derived afresh, then updated through blobs[1 ..] the way rdx_tlas_update updates a device's layout -- with the owner words
// and the wide tail written into the host arrays.  A step the update hands back (return 1), or whose blob does not keep the
// previous one's BLAS region, is derived in full.  path_per_step (optional, count - 1 entries): 1 incremental, 2 full.
static int layout_chain(const char* who, const void* const* blobs, const size_t* sizes, uint32_t count, int quad, int cull, AccelLayout& L,
                        uint32_t* path_per_step)
{
    if (!blobs || !sizes || !count) return fail("%s: no blobs", who);
    for (uint32_t i = 0; i < count; ++i) if (!blobs[i] || sizes[i] < 16) return fail("%s: blob %u is missing", who, i);
    std::string err;
    const AccelOptions opt{quad, cull};
    if (derive_accel_layout(blobs[0], sizes[0], opt, L, err)) return fail_str(err);
    auto region = [&](uint32_t i, uint32_t nInst, const uint8_t*& p, size_t& n) {
        const auto* h = static_cast<const BlobTopHeader*>(blobs[i]);
        const size_t start = (size_t)h->instByteOffset + (size_t)nInst * sizeof(BlobInst);
        if (start > sizes[i] || h->totalBufferSize > sizes[i] || h->totalBufferSize < start) return false;
        p = static_cast<const uint8_t*>(blobs[i]) + start; n = h->totalBufferSize - start;
        return true;
    };
    for (uint32_t i = 1; i < count; ++i) {
        const uint8_t* a = nullptr; const uint8_t* b = nullptr; size_t na = 0, nb = 0;
        int rc = 1;
        if (region(i - 1, L.s.nInst, a, na) && region(i, L.s.nInst, b, nb) && na == nb && std::memcmp(a, b, na) == 0) {
            AccelUpdate upd;
            rc = update_accel_layout(blobs[i], sizes[i], opt, L, upd, err);
            if (rc < 0) return fail_str(err);
            if (rc == 0) apply_accel_update(L, upd);
        }
        if (rc == 1 && derive_accel_layout(blobs[i], sizes[i], opt, L, err)) return fail_str(err);
        if (path_per_step) path_per_step[i - 1] = rc == 0 ? 1u : 2u;
    }
    return 0;
}

extern "C" int rdx_debug_accel_layout_update(const void* const* blobs, const size_t* sizes, uint32_t count, int quad, int cull,
                                             rdx_accel_scalars* scalars, void* const* arrays, size_t* bytes, uint32_t* path_per_step)
{
    if (arrays && !bytes) return fail("rdx_debug_accel_layout_update: arrays need their capacities in bytes[]");
    AccelLayout L;
    if (layout_chain("rdx_debug_accel_layout_update", blobs, sizes, count, quad, cull, L, path_per_step)) return -1;
    return export_layout(L, scalars, arrays, bytes);
}

extern "C" int rdx_debug_accel_entries(const void* const* blobs, const size_t* sizes, uint32_t count, int quad, int cull,
                                       void* entries, size_t* bytes, uint32_t* need)
{
    if (!bytes) return fail("rdx_debug_accel_entries: the capacity of `entries` goes in *bytes");
    AccelLayout L;
    if (layout_chain("rdx_debug_accel_entries", blobs, sizes, count, quad, cull, L, nullptr)) return -1;
    const size_t n = L.entries.size() * sizeof(DQuad);
    if (entries) {
        if (*bytes < n) return fail("rdx_debug_accel_entries: the entry records need %zu bytes", n);
        if (n) std::memcpy(entries, L.entries.data(), n);
    }
    *bytes = n;
    if (need) *need = L.entryNeed;
    return 0;
}

static int export_layout(const AccelLayout& L, rdx_accel_scalars* scalars, void* const* arrays, size_t* bytes)
{
    if (scalars) *scalars = L.s;
    auto view = [](const auto& v) { return std::make_pair(static_cast<const void*>(v.data()), v.size() * sizeof(v[0])); };
    const std::pair<const void*, size_t> arr[8] = {view(L.tnodes), view(L.ctnodes), view(L.insts), view(L.bnodes), view(L.tris), view(L.wide),
                                                   view(L.quad), {L.groupBits, sizeof L.groupBits}};
    for (int i = 0; i < 8 && bytes; ++i) {
        if (arrays && arrays[i]) {
            if (bytes[i] < arr[i].second) return fail("rdx_debug_accel_layout: array %d needs %zu bytes", i, arr[i].second);
            if (arr[i].second) std::memcpy(arrays[i], arr[i].first, arr[i].second);
        }
        bytes[i] = arr[i].second;
    }
    return 0;
}

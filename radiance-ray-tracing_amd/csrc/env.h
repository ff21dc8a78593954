// env.h -- the records and the launch declarations of the environment calls (env.hip): rdx_env_build, rdx_env_light_hits,
// rdx_env_lookup and rdx_trace_paths_env.  The environment is a lat-long image of float4 texels (row 0 the zenith, +y) and a
// sampling table that rdx_env_build derives from it on the device (include/rdx.h):
//
//   header 64 B | rowCos[H + 1] float32 | C[H][W] uint32 | M[H] uint64        every part 16-byte aligned
//
// rowCos[y] = (float)cos(pi y / H) is computed by the host in double and uploaded: rows are bands of cos(theta), so a texel's solid
// angle is twoPiOverW * (rowCos[y] - rowCos[y + 1]) and the device evaluates no transcendental for the table or for E.  C holds the
// inclusive prefix sums of the quantised weights q along each row, M those of the row sums; max and integer sums do not depend
// on the order they are taken in, so the table's bytes are a function of the image alone.  The streams of a bounce and its fold
// kernel are those of rdx_trace_paths_lights (light_paths.h), unchanged.  The layout functions are host and device code.
#pragma once
#include <stdint.h>

#include "area.h"
#include "light_paths.h"
#include "rdx_types.h"
#include "shade.h"

namespace rdx {

constexpr uint32_t ENV_MAGIC = 0x56454452u;        // "RDEV"
constexpr uint32_t ENV_VERSION = 1u;
constexpr uint32_t ENV_MAX_WIDTH = 16384u, ENV_MAX_HEIGHT = 8192u;
constexpr uint32_t ENV_QMAX = 65535u;              // a texel's largest quantised weight: a row sums to less than 2^30
// the lobe a scatter sample was drawn from (rdx_env_mis_weights); NONE: a direction the environment's table gave
constexpr uint32_t LOBE_DIFFUSE = 0u, LOBE_SPECULAR = 1u, LOBE_TRANSMISSION = 2u, LOBE_NONE = 3u;

struct EnvHeader {
    uint32_t magic, version, width, height;
    float wmax, twoPiOverW, wOverTwoPi;
    uint32_t _0;
    uint64_t total;
    uint32_t _1[6];
};
static_assert(sizeof(EnvHeader) == 64, "environment table header");

#if defined(__HIPCC__)
#define RDX_ENV_HD __host__ __device__
#else
#define RDX_ENV_HD
#endif
RDX_ENV_HD inline size_t env_align16(size_t bytes) { return (bytes + 15) & ~(size_t)15; }
RDX_ENV_HD inline size_t env_rowcos_offset() { return sizeof(EnvHeader); }
RDX_ENV_HD inline size_t env_c_offset(uint32_t h) { return env_rowcos_offset() + env_align16(((size_t)h + 1) * sizeof(float)); }
RDX_ENV_HD inline size_t env_m_offset(uint32_t w, uint32_t h) { return env_c_offset(h) + env_align16((size_t)w * h * sizeof(uint32_t)); }
// 0: a size outside the limits
RDX_ENV_HD inline size_t env_table_size(uint32_t w, uint32_t h)
{
    if (w < 1u || w > ENV_MAX_WIDTH || h < 1u || h > ENV_MAX_HEIGHT) return 0;
    return env_m_offset(w, h) + env_align16((size_t)h * sizeof(uint64_t));
}
#undef RDX_ENV_HD

#if defined(__HIPCC__)
// what a kernel is given of an environment: the image, the table, and the size the CALL states -- the host has checked the two
// ranges for that size, and every address a kernel forms is one of image[0 .. W H), rowCos[0 .. H], C[0 .. W H), M[0 .. H) for
// it, whatever the table holds
struct EnvView {
    const float4* image;
    const char* table;
    uint32_t W, H;
    __device__ __forceinline__ const EnvHeader* header() const { return reinterpret_cast<const EnvHeader*>(table); }
    __device__ __forceinline__ const float* rowCos() const { return reinterpret_cast<const float*>(table + env_rowcos_offset()); }
    __device__ __forceinline__ const uint32_t* C() const { return reinterpret_cast<const uint32_t*>(table + env_c_offset(H)); }
    __device__ __forceinline__ const uint64_t* M() const { return reinterpret_cast<const uint64_t*>(table + env_m_offset(W, H)); }
};

// rdx_env_build after the host has written the header (wmax = 0, total = 0) and rowCos: three launches in stream order --
// the maximum weight into header.wmax, q and its row scans into C with the row sums into M, the scan of M with header.total
void launch_env_build(hipStream_t st, const float4* image, char* table, uint32_t w, uint32_t h);
// rdx_env_light_hits: rdx_area_light_hits (area.h) with the environment in the place of the one record; of the randoms x, y, z
// are read
void launch_env_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const EnvView& env, const uint4* keys,
                           uint32_t stream, const float4* randoms, float4* lit, float4* shadow);
// rdx_env_lookup: the texel the environment shows along the direction of each of n rays (rgb, 0); zeros for a zero or non-finite
// direction and for a table whose header is not the call's
void launch_env_lookup(hipStream_t st, const float4* rays, uint32_t n, const EnvView& env, float4* radiance);
// k_env_shade: launch_area_shade (area.h) with the environment as one more record after the nLights punctual and nArea area
// records, on stream nArea: nLights + nArea + 1 records per survivor; a depth-0 miss shows the environment
void launch_env_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                      uint32_t nLights, const AreaLight* area, uint32_t nArea, const EnvView& env, const LightPathStreams& io, uint32_t n, uint32_t depth,
                      bool sampleNext, uint32_t* live, uint32_t* invalid);

// ---- multiple-importance sampling of the environment against the scatter sample (env_mis.hip; the estimator is env_mis.h) ----
// rdx_env_mis_weights: direction k = dirs[2k + 1] seen from ray / material record s = src ? src[k] : k, a record of zeros for s >=
// nrecords; the lobe from keys[s] or randoms[s], NONE where both are null; out[k] = (w, pdf_scatter, pdf_env, lobe)
void launch_env_mis_weights(hipStream_t st, const float4* rays, const float4* materials, const float4* dirs, uint32_t n, const uint32_t* src,
                            uint32_t nrecords, const uint4* keys, const float4* randoms, const EnvView& env, uint4* out);
// k_env_mis_shade: launch_env_shade with the environment's record weighted by 1 - w of its direction, w of the sampled direction in
// foldF.w, and the weighted texel of a live ray of depth > 0 without a valid hit added to radiance[path]
void launch_env_mis_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                          uint32_t nLights, const AreaLight* area, uint32_t nArea, const EnvView& env, const LightPathStreams& io, uint32_t n,
                          uint32_t depth, bool sampleNext, uint32_t* live, uint32_t* invalid);
// k_env_mis_fold: launch_lights_fold (light_paths.h) with foldF.w handed on in nWeight.w, the next live ray's weight word
void launch_env_mis_fold(hipStream_t st, const float4* any, uint32_t nLights, const LightPathStreams& io, uint32_t live);
#endif

} // namespace rdx

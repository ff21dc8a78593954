// radiance.h -- the Radiance host API (`namespace RD`) as a thin inline C++ layer over the C ABI of
// librdx.so (include/rdx.h).  Same names, signatures and error behaviour as the reference's
// radiance/include/radiance.h (:86-174), so its callers (samples/sample1.cpp, tools/sceneBuilder.cpp)
// build against this header unchanged; underneath, TraceRays runs the hand-written HIP wavefront
// path tracer instead of an OpenCL megakernel.
#pragma once

#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "core.h"
#include "clcontext.h"

#ifndef SHADER_LIB_PATH
#define SHADER_LIB_PATH ""      // the reference passes -I<this> to its OpenCL JIT; so does the run-time compilation of user shader programs
#endif

namespace RD
{

typedef void* Handle;
typedef cl_mem TopAccelStruct;
typedef cl_mem Image;
typedef cl_mem ImageArray;
typedef cl_sampler Sampler;
typedef unsigned int Uniform;
typedef cl_mem Buffer;

enum DescriptorType { ACCEL_STRUCT_TYPE, IMAGE_TYPE, IMAGE_ARRAY_TYPE, IMAGE_SAMPLER_TYPE, BUFFER_TYPE, TEX_ARRAY_TYPE };

struct Mesh { std::vector<Vec3> vertexData; std::vector<Triangle> indexData; };

struct BVHNode;
struct _BottomAccelStruct { BVHNode* root; std::vector<char> data; rdx_blas handle; };
typedef _BottomAccelStruct* BottomAccelStruct;

struct Instance
{
    Mat4x4 transform;                 // row-major object->world
    unsigned int SBTOffset;
    unsigned int customInstanceID;
    BottomAccelStruct bottomAccelStruct;
};

typedef std::vector<Handle> DescriptorSet;
typedef std::vector<DescriptorType> PipelineLayout;
typedef cl_kernel ShaderModule;

#define SHADER_UNUSED (~0U)
struct ShaderGroup { ShaderModule generalShader, closestHitShader, anyHitShader; };
struct PipelineCreateInfo
{
    unsigned int maxRayRecursionDepth;
    PipelineLayout layout;
    std::vector<ShaderModule> modules;
    std::vector<ShaderGroup> groups;
};
typedef PipelineCreateInfo Pipeline;

#define CHANNEL 4
#define RD_CHANNEL CHANNEL

typedef uint32_t AddressingMode;
#define RD_ADDRESS_CLAMP_TO_EDGE CL_ADDRESS_CLAMP_TO_EDGE
#define RD_ADDRESS_CLAMP CL_ADDRESS_CLAMP
#define RD_ADDRESS_REPEAT CL_ADDRESS_REPEAT
#define RD_ADDRESS_MIRRORED_REPEAT CL_ADDRESS_MIRRORED_REPEAT
typedef uint32_t FilterMode;
#define RD_FILTER_NEAREST CL_FILTER_NEAREST
#define RD_FILTER_LINEAR CL_FILTER_LINEAR

struct Platform
{
    static Platform* GetPlatform()
    {
        static Platform ctx;
        if (!ctx.initialized) {
            ctx.clContext = CLContext::GetCLContext();
            ctx.initialized = true;
            printf("Platform initialized.\n");
        }
        return &ctx;
    }
    ~Platform() { printf("Platform destroyed.\n"); if (clContext) clContext->Cleanup(); }

    Pipeline activePipeline;
    CLContext* clContext = nullptr;
    bool initialized = false;

private:
    Platform() = default;
    void operator=(Platform&) = delete;
    Platform(Platform&) = delete;
};

namespace detail
{
[[noreturn]] inline void fatal(const char* what)
{
    printf("Radiance Error: %s: %s\n", what, rdx_last_error());
    rdx_shutdown();
    exit(-1);
}
template <class T> inline T* need(T* p, const char* what) { if (!p) fatal(what); return p; }
} // namespace detail

// ---- acceleration structures (blocking) -----------------------------------------------------------
inline BottomAccelStruct BuildAccelStruct(Platform*, Mesh& mesh)
{
    printf("\nStart building bottom level BVH\n\tVertex count:%ld\n\tTriangle count:%ld\n", (long)mesh.vertexData.size(),
           (long)mesh.indexData.size());
    static_assert(sizeof(Vec3) == 12 && sizeof(Triangle) == 12, "Mesh element layout");
    rdx_blas h = detail::need(rdx_blas_build(reinterpret_cast<const float*>(mesh.vertexData.data()), (uint32_t)mesh.vertexData.size(),
                                             reinterpret_cast<const uint32_t*>(mesh.indexData.data()), (uint32_t)mesh.indexData.size()),
                              "BuildAccelStruct(Mesh)");
    _BottomAccelStruct* as = new _BottomAccelStruct();
    as->root = nullptr;
    as->handle = h;
    uint32_t n = 0;
    const char* p = static_cast<const char*>(rdx_blas_data(h, &n));
    as->data.assign(p, p + n);
    printf("Max BVH depth is %d\n", rdx_blas_max_depth(h));
    return as;
}

namespace detail
{
inline std::vector<rdx_instance> instances_in(std::vector<Instance>& instances)
{
    std::vector<rdx_instance> in(instances.size());
    for (size_t i = 0; i < instances.size(); ++i) {
        const float* m = &instances[i].transform.a1;
        for (int k = 0; k < 16; ++k) in[i].transform[k] = m[k];
        in[i].SBTOffset = instances[i].SBTOffset;
        in[i].customInstanceID = instances[i].customInstanceID;
        in[i].bottomAccelStruct = instances[i].bottomAccelStruct ? instances[i].bottomAccelStruct->handle : nullptr;
    }
    return in;
}
} // namespace detail

inline TopAccelStruct BuildAccelStruct(Platform*, std::vector<Instance>& instances)
{
    printf("\nStart building top level BVH\n\tInstance count: %ld\n", (long)instances.size());
    std::vector<rdx_instance> in = detail::instances_in(instances);
    return detail::need(rdx_tlas_build(in.data(), (uint32_t)in.size()), "BuildAccelStruct(instances)");
}

// Extension (no reference counterpart; rdx_tlas_update): other transforms, SBT offsets or custom ids for the instances
// `accelStruct` was built from -- same count, same bottom-level structure at every index.  The handle stays valid and bound.
inline void UpdateAccelStruct(Platform*, TopAccelStruct accelStruct, std::vector<Instance>& instances)
{
    std::vector<rdx_instance> in = detail::instances_in(instances);
    if (rdx_tlas_update(accelStruct, in.data(), (uint32_t)in.size())) detail::fatal("UpdateAccelStruct");
}

inline void TopAccelStructToFile(Platform*, TopAccelStruct accelStruct, const char* path) { if (rdx_tlas_to_file(accelStruct, path)) detail::fatal("TopAccelStructToFile"); }
inline void FileToTopAccelStruct(Platform*, const char* path, TopAccelStruct* accelStruct) { *accelStruct = detail::need(rdx_tlas_from_file(path), "FileToTopAccelStruct"); }

// Extension (no reference counterpart; rdx_resolve_hits): surface records (rdx_surface: world-space hit point, normal, the two
// offset origins, uv, material number) for the `n` records `hits` that rdx_query_rays(..., RDX_QUERY_CLOSEST, ...) wrote for `rays`,
// device memory in and out.  `scene` = the buffers bound to descriptor slots 5, 7, 8, 9.  Returns the number of records the bounds
// rule refused (they are written as zeros).
inline uint32_t ResolveHits(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer hits, uint32_t n, const rdx_surface_buffers& scene,
                            Buffer out, size_t raysOffset = 0, size_t hitsOffset = 0, size_t outOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_resolve_hits(accelStruct, rays, raysOffset, hits, hitsOffset, n, &scene, out, outOffset, &invalid)) detail::fatal("ResolveHits");
    return invalid;
}

// Extension (no reference counterpart; rdx_shade_hits): the stock closest-hit / miss shaders on the `n` records `hits` that
// rdx_query_rays(..., RDX_QUERY_CLOSEST, ...) wrote for `rays`, with `keys` (rdx_shade_key) as the RNG inputs; device memory in and out.
// `scene` = the buffers bound to descriptor slots 4, 5, 7, 8, 9, 10, 11, 12.  One rdx_shade per ray goes to `shade`; `next` / `shadow`
// (each may be nullptr) receive the next ray and the shadow ray of every surviving ray, `src` (may be nullptr) switches compaction
// on and receives the surviving rays' numbers.  Returns the number of surviving rays; *invalid (optional): records the bounds rule
// refused.
inline uint32_t ShadeHits(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer hits, Buffer keys, uint32_t n, const rdx_shading_buffers& scene,
                          Buffer shade, Buffer next, Buffer shadow, Buffer src, uint32_t* invalid = nullptr, size_t raysOffset = 0,
                          size_t hitsOffset = 0, size_t keysOffset = 0, size_t shadeOffset = 0, size_t nextOffset = 0, size_t shadowOffset = 0,
                          size_t srcOffset = 0)
{
    uint32_t live = 0;
    if (rdx_shade_hits(accelStruct, rays, raysOffset, hits, hitsOffset, keys, keysOffset, n, &scene, shade, shadeOffset, next, nextOffset, shadow,
                       shadowOffset, src, srcOffset, &live, invalid))
        detail::fatal("ShadeHits");
    return live;
}

// Extension (no reference counterpart; rdx_resolve_materials): the evaluated material (rdx_material_record: shading normal, albedo,
// metallic, roughness, transmission, ior, the shadow ray's origin, material number) of the `n` records `hits` that
// rdx_query_rays(..., RDX_QUERY_CLOSEST, ...) wrote for `rays`, device memory in and out.  `scene` as for ShadeHits.  Returns the number
// of records the bounds rule refused (they are written as zeros).
inline uint32_t ResolveMaterials(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer hits, uint32_t n, const rdx_shading_buffers& scene,
                                 Buffer out, size_t raysOffset = 0, size_t hitsOffset = 0, size_t outOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_resolve_materials(accelStruct, rays, raysOffset, hits, hitsOffset, n, &scene, out, outOffset, &invalid)) detail::fatal("ResolveMaterials");
    return invalid;
}

// Extension (no reference counterpart; rdx_light_hits): the direct term of directional light `light` (0 .. 4) of the SceneProperties
// in `scene` (the buffer of descriptor slot 4) for the `n` material records `materials` and the directions of `rays`: one float4
// (rgb, 0) per ray goes to `lit`, the shadow ray towards the light (rdx_ray, ready for rdx_query_rays(..., RDX_QUERY_ANY, ...)) to
// `shadow` (may be nullptr).  The ambient term stays the caller's.
inline void LightHits(Platform*, Buffer rays, Buffer materials, uint32_t n, Buffer scene, uint32_t light, Buffer lit, Buffer shadow = nullptr,
                      size_t raysOffset = 0, size_t materialsOffset = 0, size_t litOffset = 0, size_t shadowOffset = 0)
{
    if (rdx_light_hits(rays, raysOffset, materials, materialsOffset, n, scene, light, lit, litOffset, shadow, shadowOffset)) detail::fatal("LightHits");
}

// Extension (no reference counterpart; rdx_punctual_light_hits): LightHits for record `index` of the caller's light table `lights`
// (rdx_punctual_light records in device memory, the first at lightsOffset): directional, point or spot.  The shadow ray towards a
// point or spot light ends at the light; a record that is dark at a hit gives zeros in `lit` and `shadow`.
inline void PunctualLightHits(Platform*, Buffer rays, Buffer materials, uint32_t n, Buffer lights, uint32_t index, Buffer lit, Buffer shadow = nullptr,
                              size_t raysOffset = 0, size_t materialsOffset = 0, size_t lightsOffset = 0, size_t litOffset = 0, size_t shadowOffset = 0)
{
    if (rdx_punctual_light_hits(rays, raysOffset, materials, materialsOffset, n, lights, lightsOffset + sizeof(rdx_punctual_light) * (size_t)index, lit,
                                litOffset, shadow, shadowOffset))
        detail::fatal("PunctualLightHits");
}

// Extension (no reference counterpart; rdx_scatter_hits): the next ray of the `n` material records `materials` (rdx_resolve_materials')
// and surface records `surfaces` (rdx_resolve_hits') and the directions of `rays` -- the stock shader's next-direction sample, with
// pcg3d of the rdx_shade_key records `keys` as the random numbers, or with the float4 records `randoms` (exactly one of the two is
// nullptr).  One rdx_scatter (nextFactor, slot) per ray goes to `scatter`, the next ray of every survivor (rdx_ray, ready for
// rdx_query_rays) to `next`; with `src` (may be nullptr) the survivors are packed and src[k] is the ray's number.  Returns the
// number of survivors.
inline uint32_t ScatterHits(Platform*, Buffer rays, Buffer materials, Buffer surfaces, Buffer keys, Buffer randoms, uint32_t n, Buffer scatter,
                            Buffer next, Buffer src = nullptr, size_t raysOffset = 0, size_t materialsOffset = 0, size_t surfacesOffset = 0,
                            size_t keysOffset = 0, size_t randomsOffset = 0, size_t scatterOffset = 0, size_t nextOffset = 0, size_t srcOffset = 0)
{
    uint32_t live = 0;
    if (rdx_scatter_hits(rays, raysOffset, materials, materialsOffset, surfaces, surfacesOffset, keys, keysOffset, randoms, randomsOffset, n,
                         scatter, scatterOffset, next, nextOffset, src, srcOffset, &live))
        detail::fatal("ScatterHits");
    return live;
}

// Extension (no reference counterpart; rdx_generate_rays): `n` camera rays of the PhysicalCamera in `camera` (the contents of
// descriptor slot 3) as rdx_ray records in `rays`, and -- `keys` may be nullptr -- their rdx_shade_key records of depth 0; device
// memory in and out.  Ray i is pixel firstPixel + i, or pixels[i]; its random input is pcg3d(frameID, totalSamples, pixel), or
// pcg3d of seeds[i] (rdx_raygen_seed).  pixels / seeds may be nullptr.
inline void GenerateRays(Platform*, Buffer camera, uint32_t n, uint32_t frameID, uint32_t totalSamples, Buffer rays, Buffer keys,
                         uint32_t firstPixel = 0, Buffer pixels = nullptr, Buffer seeds = nullptr, float tmin = 0.001f, float tmax = 1000.0f,
                         size_t pixelsOffset = 0, size_t seedsOffset = 0, size_t raysOffset = 0, size_t keysOffset = 0)
{
    if (rdx_generate_rays(camera, n, firstPixel, pixels, pixelsOffset, frameID, totalSamples, seeds, seedsOffset, tmin, tmax, rays, raysOffset,
                          keys, keysOffset))
        detail::fatal("GenerateRays");
}

// Extension (no reference counterpart; rdx_accumulate): sample `frameID` of `n` distinct pixels (firstPixel + i, or pixels[i]),
// float4 colours in `colors`, folded into imageScratch by the reference's running mean; `image` (may be nullptr) receives the
// tone-mapped RGBA8 of those pixels (debug: no ACES, no gamma).  Returns the samples whose pixel lies outside the frame.
inline uint32_t Accumulate(Platform*, Buffer colors, uint32_t n, uint32_t frameID, Buffer imageScratch, Image image = nullptr,
                           uint32_t firstPixel = 0, Buffer pixels = nullptr, bool debug = false, size_t colorsOffset = 0, size_t pixelsOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_accumulate(colors, colorsOffset, n, firstPixel, pixels, pixelsOffset, frameID, imageScratch, image, debug ? RDX_ACCUMULATE_DEBUG : 0u,
                       &invalid))
        detail::fatal("Accumulate");
    return invalid;
}

// Extension (no reference counterpart; rdx_trace_paths): radiance along `n` rays of the caller's own -- the reference's raygen
// loop from ray i (rdx_ray, its own tmin / tmax for the first segment) with keys[i] (rdx_shade_key: frameID, pixel) to the depth
// `maxDepth`, on the frame path's stages; one float4 (rgb, 0) per ray goes to `radiance`, the first segment's rdx_ray_hit records
// to `hits` (may be nullptr); device memory in and out.  `scene` = the buffers bound to descriptor slots 4, 5, 7, 8, 9, 10, 11, 12;
// they must describe the scene of `accelStruct` (rdx.h).
inline void TracePaths(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer keys, uint32_t n, uint32_t maxDepth, const rdx_shading_buffers& scene,
                       Buffer radiance, Buffer hits = nullptr, size_t raysOffset = 0, size_t keysOffset = 0, size_t radianceOffset = 0,
                       size_t hitsOffset = 0)
{
    if (rdx_trace_paths(accelStruct, rays, raysOffset, keys, keysOffset, n, maxDepth, &scene, radiance, radianceOffset, hits, hitsOffset))
        detail::fatal("TracePaths");
}

// Extension (no reference counterpart; rdx_trace_paths_lights): TracePaths with every one of the first `lightCount` (0 .. 5)
// directional lights of the scene's SceneProperties sampled at every hit -- the path tracer over ResolveHits / ResolveMaterials /
// LightHits / ScatterHits in one call, device memory in and out.  Gathers checked: returns the number of hits that `scene` does not
// describe (they count as misses).  With lightCount 1 the result has the bits of TracePaths (rdx.h).
inline uint32_t TraceLightPaths(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer keys, uint32_t n, uint32_t maxDepth, uint32_t lightCount,
                                const rdx_shading_buffers& scene, Buffer radiance, size_t raysOffset = 0, size_t keysOffset = 0,
                                size_t radianceOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_trace_paths_lights(accelStruct, rays, raysOffset, keys, keysOffset, n, maxDepth, lightCount, &scene, radiance, radianceOffset, &invalid))
        detail::fatal("TraceLightPaths");
    return invalid;
}

// Extension (no reference counterpart; rdx_trace_paths_punctual): TraceLightPaths with the first `lightCount` (0 ..
// RDX_MAX_PATH_LIGHTS) records of the caller's light table `lights` sampled at every hit in the place of the scene's directional
// lights -- the path tracer over ResolveHits / ResolveMaterials / PunctualLightHits / ScatterHits in one call.  Returns the number
// of hits that `scene` does not describe (they count as misses).
inline uint32_t TracePunctualPaths(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer keys, uint32_t n, uint32_t maxDepth, Buffer lights,
                                   uint32_t lightCount, const rdx_shading_buffers& scene, Buffer radiance, size_t raysOffset = 0, size_t keysOffset = 0,
                                   size_t lightsOffset = 0, size_t radianceOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_trace_paths_punctual(accelStruct, rays, raysOffset, keys, keysOffset, n, maxDepth, lights, lightsOffset, lightCount, &scene, radiance,
                                 radianceOffset, &invalid))
        detail::fatal("TracePunctualPaths");
    return invalid;
}

// Extension (no reference counterpart; rdx_area_light_hits): PunctualLightHits for record `index` of the caller's AREA light table
// `lights` (rdx_area_light records in device memory, the first at lightsOffset): a quad or a triangle, sampled at one point per
// ray with pcg3d of the rdx_shade_key records `keys` on random stream `stream`, or with x and y of the float4 records `randoms`
// (exactly one of the two is nullptr).  The shadow ray stops short of the emitter; a record that is dark at a hit gives zeros.
inline void AreaLightHits(Platform*, Buffer rays, Buffer materials, uint32_t n, Buffer lights, uint32_t index, Buffer keys, uint32_t stream, Buffer randoms,
                          Buffer lit, Buffer shadow = nullptr, size_t raysOffset = 0, size_t materialsOffset = 0, size_t lightsOffset = 0,
                          size_t keysOffset = 0, size_t randomsOffset = 0, size_t litOffset = 0, size_t shadowOffset = 0)
{
    if (rdx_area_light_hits(rays, raysOffset, materials, materialsOffset, n, lights, lightsOffset + sizeof(rdx_area_light) * (size_t)index, keys, keysOffset,
                            stream, randoms, randomsOffset, lit, litOffset, shadow, shadowOffset))
        detail::fatal("AreaLightHits");
}

// Extension (no reference counterpart; rdx_trace_paths_area): TracePunctualPaths over two tables -- the first `lightCount` records
// of `lights`, then the first `areaCount` rdx_area_light records of `area` (record j on random stream j), lightCount + areaCount
// <= RDX_MAX_PATH_LIGHTS; a table of no records may be nullptr.  The emitters are not geometry: no ray sees them.  Returns the
// number of hits that `scene` does not describe (they count as misses).
inline uint32_t TraceAreaPaths(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer keys, uint32_t n, uint32_t maxDepth, Buffer lights,
                               uint32_t lightCount, Buffer area, uint32_t areaCount, const rdx_shading_buffers& scene, Buffer radiance,
                               size_t raysOffset = 0, size_t keysOffset = 0, size_t lightsOffset = 0, size_t areaOffset = 0, size_t radianceOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_trace_paths_area(accelStruct, rays, raysOffset, keys, keysOffset, n, maxDepth, lights, lightsOffset, lightCount, area, areaOffset, areaCount,
                             &scene, radiance, radianceOffset, &invalid))
        detail::fatal("TraceAreaPaths");
    return invalid;
}

// Extension (no reference counterpart; rdx_env_table_size, rdx_env_build): the bytes of the sampling table of a width x height
// lat-long environment image (0: a size outside the limits), and the table of the float4 image `image` built into `table`.
inline size_t EnvTableSize(uint32_t width, uint32_t height) { return rdx_env_table_size(width, height); }
inline void BuildEnvironment(Platform*, Buffer image, uint32_t width, uint32_t height, Buffer table, size_t imageOffset = 0, size_t tableOffset = 0)
{
    if (rdx_env_build(image, imageOffset, width, height, table, tableOffset))
        detail::fatal("BuildEnvironment");
}

// Extension (no reference counterpart; rdx_env_light_hits): AreaLightHits with the environment (image + table) in the place of the
// one record: one importance-sampled direction per ray, from pcg3d of `keys` on random stream `stream` or from x, y, z of `randoms`
// (exactly one of the two is nullptr).  The shadow ray has the stock interval; an environment without light gives zeros.
inline void EnvLightHits(Platform*, Buffer rays, Buffer materials, uint32_t n, Buffer image, Buffer table, uint32_t width, uint32_t height, Buffer keys,
                         uint32_t stream, Buffer randoms, Buffer lit, Buffer shadow = nullptr, size_t raysOffset = 0, size_t materialsOffset = 0,
                         size_t imageOffset = 0, size_t tableOffset = 0, size_t keysOffset = 0, size_t randomsOffset = 0, size_t litOffset = 0,
                         size_t shadowOffset = 0)
{
    if (rdx_env_light_hits(rays, raysOffset, materials, materialsOffset, n, image, imageOffset, table, tableOffset, width, height, keys, keysOffset, stream,
                           randoms, randomsOffset, lit, litOffset, shadow, shadowOffset))
        detail::fatal("EnvLightHits");
}

// Extension (no reference counterpart; rdx_env_lookup): the texel (rgb, 0) the environment shows along the direction of each ray.
inline void EnvLookup(Platform*, Buffer rays, uint32_t n, Buffer image, Buffer table, uint32_t width, uint32_t height, Buffer radiance,
                      size_t raysOffset = 0, size_t imageOffset = 0, size_t tableOffset = 0, size_t radianceOffset = 0)
{
    if (rdx_env_lookup(rays, raysOffset, n, image, imageOffset, table, tableOffset, width, height, radiance, radianceOffset))
        detail::fatal("EnvLookup");
}

// Extension (no reference counterpart; rdx_trace_paths_env): TraceAreaPaths with the environment as one more record after the two
// tables (random stream areaCount), lightCount + areaCount + 1 <= RDX_MAX_PATH_LIGHTS; a first ray that hits nothing shows the
// environment.  Returns the number of hits that `scene` does not describe (they count as misses).
inline uint32_t TraceEnvPaths(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer keys, uint32_t n, uint32_t maxDepth, Buffer lights,
                              uint32_t lightCount, Buffer area, uint32_t areaCount, Buffer image, Buffer table, uint32_t width, uint32_t height,
                              const rdx_shading_buffers& scene, Buffer radiance, size_t raysOffset = 0, size_t keysOffset = 0, size_t lightsOffset = 0,
                              size_t areaOffset = 0, size_t imageOffset = 0, size_t tableOffset = 0, size_t radianceOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_trace_paths_env(accelStruct, rays, raysOffset, keys, keysOffset, n, maxDepth, lights, lightsOffset, lightCount, area, areaOffset, areaCount, image,
                            imageOffset, table, tableOffset, width, height, &scene, radiance, radianceOffset, &invalid))
        detail::fatal("TraceEnvPaths");
    return invalid;
}

// Extension (no reference counterpart; rdx_env_mis_weights): the balance-heuristic weight of the scatter sample against the
// environment's for the directions of the n rdx_ray records of `dirs` (EnvLightHits' shadow rays, ScatterHits' next rays), seen from
// record src[k] (src nullptr: k, and nrecords == n) of the nrecords rays / materials; keys or randoms as given to ScatterHits (at
// most one; both nullptr: the environment's own direction).  One rdx_env_mis_weight per direction to `out`.
inline void EnvMisWeights(Platform*, Buffer rays, Buffer materials, Buffer dirs, uint32_t n, Buffer src, uint32_t nrecords, Buffer keys, Buffer randoms,
                          Buffer image, Buffer table, uint32_t width, uint32_t height, Buffer out, size_t raysOffset = 0, size_t materialsOffset = 0,
                          size_t dirsOffset = 0, size_t srcOffset = 0, size_t keysOffset = 0, size_t randomsOffset = 0, size_t imageOffset = 0,
                          size_t tableOffset = 0, size_t outOffset = 0)
{
    if (rdx_env_mis_weights(rays, raysOffset, materials, materialsOffset, dirs, dirsOffset, n, src, srcOffset, nrecords, keys, keysOffset, randoms,
                            randomsOffset, image, imageOffset, table, tableOffset, width, height, out, outOffset))
        detail::fatal("EnvMisWeights");
}

// Extension (no reference counterpart; rdx_trace_paths_env_mis): TraceEnvPaths with the environment and the scatter sample weighted
// against each other: a bounce ray that leaves the scene shows the environment, so mirrors and glass see the sky.
inline uint32_t TraceEnvMisPaths(Platform*, TopAccelStruct accelStruct, Buffer rays, Buffer keys, uint32_t n, uint32_t maxDepth, Buffer lights,
                                 uint32_t lightCount, Buffer area, uint32_t areaCount, Buffer image, Buffer table, uint32_t width, uint32_t height,
                                 const rdx_shading_buffers& scene, Buffer radiance, size_t raysOffset = 0, size_t keysOffset = 0, size_t lightsOffset = 0,
                                 size_t areaOffset = 0, size_t imageOffset = 0, size_t tableOffset = 0, size_t radianceOffset = 0)
{
    uint32_t invalid = 0;
    if (rdx_trace_paths_env_mis(accelStruct, rays, raysOffset, keys, keysOffset, n, maxDepth, lights, lightsOffset, lightCount, area, areaOffset, areaCount,
                                image, imageOffset, table, tableOffset, width, height, &scene, radiance, radianceOffset, &invalid))
        detail::fatal("TraceEnvMisPaths");
    return invalid;
}

// Extension (no reference counterpart; rdx_denoise_work_size, rdx_denoise): the frame's denoiser -- an edge-avoiding a-trous filter
// over the width x height float4 colours in `color`, guided by the rdx_material_record / rdx_surface records of the same pixels'
// primary hits; the result goes to `out` (float4 per pixel, w kept) and, tone-mapped as Accumulate does it, to `image` (RGBA8, may
// be nullptr).  `work` holds DenoiseWorkSize(width, height) bytes (0: a size outside the limits) of no lasting meaning.
inline size_t DenoiseWorkSize(uint32_t width, uint32_t height) { return rdx_denoise_work_size(width, height); }
inline void Denoise(Platform*, Buffer color, Buffer materials, Buffer surfaces, uint32_t width, uint32_t height, const rdx_denoise_settings& settings,
                    Buffer work, Buffer out, Image image = nullptr, size_t colorOffset = 0, size_t materialsOffset = 0, size_t surfacesOffset = 0,
                    size_t workOffset = 0, size_t outOffset = 0, size_t imageOffset = 0)
{
    if (rdx_denoise(color, colorOffset, materials, materialsOffset, surfaces, surfacesOffset, width, height, &settings, work, workOffset, out, outOffset, image,
                    imageOffset))
        detail::fatal("Denoise");
}

// Extension (no reference counterpart; rdx_camera_view, rdx_temporal_history_size, rdx_temporal_accumulate): temporal accumulation --
// CameraView writes the rdx_view of the PhysicalCamera in `camera` (as GenerateRays reads it) to `view`; TemporalAccumulate carries
// `historyIn` (may be nullptr: a history starts) through `previousView` (nullptr: the camera did not move) to the camera of `view`,
// folds the width x height float4 colours in `color` into it and writes `historyOut`: TemporalHistorySize(width, height) bytes, four
// planes of one float4 per pixel, of which plane 0 -- at historyOutOffset -- is what Denoise takes as `color`.  `previousPositions`
// (float4 per pixel, may be nullptr) says where each pixel's surface point was one frame ago; `image` (RGBA8, may be nullptr) is
// plane 0 tone-mapped as Accumulate does it.
inline void CameraView(Platform*, Buffer camera, Buffer view, size_t viewOffset = 0)
{
    if (rdx_camera_view(camera, view, viewOffset)) detail::fatal("CameraView");
}
inline size_t TemporalHistorySize(uint32_t width, uint32_t height) { return rdx_temporal_history_size(width, height); }
inline void TemporalAccumulate(Platform*, Buffer color, Buffer materials, Buffer surfaces, Buffer view, uint32_t width, uint32_t height,
                               const rdx_temporal_settings& settings, Buffer historyIn, Buffer historyOut, Buffer previousView = nullptr,
                               Buffer previousPositions = nullptr, Image image = nullptr, size_t colorOffset = 0, size_t materialsOffset = 0,
                               size_t surfacesOffset = 0, size_t viewOffset = 0, size_t historyInOffset = 0, size_t historyOutOffset = 0,
                               size_t previousViewOffset = 0, size_t previousPositionsOffset = 0, size_t imageOffset = 0)
{
    if (rdx_temporal_accumulate(color, colorOffset, materials, materialsOffset, surfaces, surfacesOffset, previousPositions, previousPositionsOffset, view,
                                viewOffset, previousView, previousViewOffset, width, height, &settings, historyIn, historyInOffset, historyOut,
                                historyOutOffset, image, imageOffset))
        detail::fatal("TemporalAccumulate");
}

// Extension (no reference counterpart; rdx_svgf_work_size, rdx_svgf_filter): the variance-guided a-trous filter of SVGF -- Denoise's
// passes with a luminance weight in units of the local standard deviation.  `color` and `moments` are typically planes 0 and 1 of a
// history TemporalAccumulate wrote: the same Buffer at colorOffset = the history's offset and momentsOffset = that + 16 width height.
// The result goes to `out` (float4 per pixel, w kept), the filtered variance to `varianceOut` (one float per pixel, may be nullptr),
// the iterate after settings.feedback_pass passes to `feedback` (float4 per pixel; given iff feedback_pass != 0: what the caller
// copies into plane 0 for the next frame) and, tone-mapped as Accumulate does it, to `image` (RGBA8, may be nullptr).  `work` holds
// SvgfWorkSize(width, height) bytes (0: a size outside the limits) of no lasting meaning.
inline size_t SvgfWorkSize(uint32_t width, uint32_t height) { return rdx_svgf_work_size(width, height); }
inline void SvgfFilter(Platform*, Buffer color, Buffer moments, Buffer materials, Buffer surfaces, uint32_t width, uint32_t height,
                       const rdx_svgf_settings& settings, Buffer work, Buffer out, Buffer varianceOut = nullptr, Buffer feedback = nullptr, Image image = nullptr,
                       size_t colorOffset = 0, size_t momentsOffset = 0, size_t materialsOffset = 0, size_t surfacesOffset = 0, size_t workOffset = 0,
                       size_t outOffset = 0, size_t varianceOutOffset = 0, size_t feedbackOffset = 0, size_t imageOffset = 0)
{
    if (rdx_svgf_filter(color, colorOffset, moments, momentsOffset, materials, materialsOffset, surfaces, surfacesOffset, width, height, &settings, work,
                        workOffset, out, outOffset, varianceOut, varianceOutOffset, feedback, feedbackOffset, image, imageOffset))
        detail::fatal("SvgfFilter");
}

// ---- resources ----------------------------------------------------------------------------------------
inline Buffer CreateBuffer(Platform*, unsigned int size) { return detail::need(rdx_buffer_create(size), "CreateBuffer"); }
inline Image CreateImage(Platform*, unsigned int width, unsigned int height) { return detail::need(rdx_buffer_create((size_t)width * height * CHANNEL), "CreateImage"); }
// texture arrays / samplers (radiance.cpp:96-137, 202-224): RGBA8 2D image arrays; sampled by the stock shader when option
// "textures" is on (the live reference shader has its reads commented out, see rdx.h)
inline ImageArray CreateImageArray(Platform*, unsigned int width, unsigned int height, unsigned int arraySize) { return detail::need(rdx_image_array_create(width, height, arraySize), "CreateImageArray"); }
inline Sampler CreateSampler(Platform*, AddressingMode addressingMode, FilterMode filterMode) { return detail::need(rdx_sampler_create(addressingMode, filterMode), "CreateSampler"); }
inline void ReadImage(Platform*, ImageArray handle, unsigned int width, unsigned int height, size_t arrayIndex, void* data) { if (rdx_image_read(handle, width, height, arrayIndex, data)) detail::fatal("ReadImage"); }
inline void WriteImage(Platform*, ImageArray handle, unsigned int width, unsigned int height, size_t arrayIndex, void* data) { if (rdx_image_write(handle, width, height, arrayIndex, data)) detail::fatal("WriteImage"); }
inline void ReadBuffer(Platform*, Buffer handle, size_t size, void* data, size_t offset = 0) { if (rdx_buffer_read(handle, offset, size, data)) detail::fatal("ReadBuffer"); }
inline void WriteBuffer(Platform*, Buffer handle, size_t size, void* data, size_t offset = 0) { if (rdx_buffer_write(handle, offset, size, data)) detail::fatal("WriteBuffer"); }

// ---- pipeline -----------------------------------------------------------------------------------------
inline DescriptorSet CreateDescriptorSet(std::vector<Handle> handles) { return handles; }
inline PipelineLayout CreatePipelineLayout(std::vector<DescriptorType> descriptorTypes) { return descriptorTypes; }
inline ShaderModule CreateShaderModule(Platform*, char* code, unsigned int size, char* name)
{
    printf("build program and get raygen kernel\n");
    if (SHADER_LIB_PATH[0]) rdx_shader_include_path(SHADER_LIB_PATH);      // the reference's clBuildProgram("-g -I" SHADER_LIB_PATH)
    return detail::need(rdx_shader_module_create(code, size, name), "CreateShaderModule");
}
inline ShaderModule CreateShaderModule(Platform* p, char* code, unsigned int size, const char* name) { return CreateShaderModule(p, code, size, const_cast<char*>(name)); }
inline Pipeline CreatePipeline(PipelineCreateInfo pipelineCreateInfo) { return pipelineCreateInfo; }
inline void BindPipeline(Platform* platform, Pipeline pipeline)
{
    platform->activePipeline = pipeline;
    if (pipeline.modules.empty() || rdx_bind_pipeline(pipeline.modules[0])) detail::fatal("BindPipeline");
}
inline void BindDescriptorSet(Platform*, DescriptorSet descriptorSet)
{
    if (rdx_bind_descriptor_set(descriptorSet.data(), (uint32_t)descriptorSet.size())) detail::fatal("BindDescriptorSet");
}
inline void TraceRays(Platform*, unsigned int raygenGroupIndex, unsigned int missGroupIndex, unsigned int hitGroupIndex,
                      unsigned int width, unsigned int height)
{
    if (rdx_trace_rays(raygenGroupIndex, missGroupIndex, hitGroupIndex, width, height)) detail::fatal("TraceRays");
}

} // namespace RD

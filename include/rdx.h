/*
 * rdx.h -- C ABI of the MI355X-native ray-tracing core ("librdx.so").
 *
 * This is the drop-in boundary for the hot path  raygen -> BVH traversal -> triangle
 * intersection -> closest-hit / any-hit / miss -> accumulate  of zekailin00/Radiance-Ray-Tracing.
 * Every entry point replaces one function of the reference's host runtime
 * (radiance/include/radiance.h, implemented over OpenCL in radiance/src/radiance.cpp); the
 * reference interface it stands in for is cited per function.  Plain pointers, sizes and POD
 * structs only -- no C++ types, no torch types.  The C++ facade `namespace RD` in
 * include/radiance.h is a thin inline layer over these calls, so reference callers
 * (samples/sample1.cpp, tools/sceneBuilder.cpp) compile against it unchanged.
 *
 * Conventions
 *   - every function that can fail returns int: 0 = OK, <0 = error (rdx_last_error() has text);
 *     constructors return a handle or NULL.  The reference never returns errors (it prints and
 *     exit(-1)s, radiance/src/clcontext.h:27-47); the RD:: facade reproduces that policy on top.
 *   - single caller thread, blocking calls (radiance.cpp:190-223 use CL_TRUE everywhere).
 *   - handles stay valid until rdx_shutdown(); nothing needs to be destroyed
 *     (the reference has no Destroy/Release calls at all, radiance.h:88-144).
 */
#ifndef RDX_H
#define RDX_H

#include <stddef.h>
#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

typedef struct rdx_buffer_s* rdx_buffer;   /* replaces RD::Buffer/Image/TopAccelStruct = cl_mem   (radiance.h:12-19) */
typedef struct rdx_blas_s*   rdx_blas;     /* replaces RD::BottomAccelStruct                     (radiance.h:52-60) */
typedef struct rdx_shader_s* rdx_shader;   /* replaces RD::ShaderModule = cl_kernel              (radiance.h:79)    */
typedef struct rdx_sampler_s* rdx_sampler; /* replaces RD::Sampler = cl_sampler                  (radiance.h:16)    */

/* Host instance record, mirrors RD::Instance (radiance.h:67-74). */
typedef struct rdx_instance {
    float    transform[16];      /* row-major object->world (aiMatrix4x4 a1..d4) */
    uint32_t SBTOffset;
    uint32_t customInstanceID;
    rdx_blas bottomAccelStruct;
} rdx_instance;

/* ---- platform: replaces RD::Platform::GetPlatform / CLContext::GetCLContext
 *      (radiance.h:146-174, radiance/src/clcontext.cpp:12-40) */
int         rdx_init(int device_ordinal);            /* idempotent; -1 = current device */
/* Single-process multi-device rendering (no reference counterpart: the reference is single-device, clcontext.cpp:17-36).  After
 * this call every buffer is replicated on `n` devices (writes go to all, reads come from logical device 0) and rdx_trace_rays
 * shards the frame by interleaved 64x64 image tiles over them -- one internal host thread per device, the caller still makes
 * one blocking call -- and copies every device's RGBA8 and imageScratch tiles into device 0's buffers before it returns.
 * ordinals[i] = HIP device of logical device i (NULL: consecutive devices starting at the one rdx_init chose).  Call before
 * creating buffers.  Results are bit-identical to one device (pixel / RNG indices stay global). */
int         rdx_init_devices(uint32_t n, const int* ordinals);
int         rdx_device_count(void);
int         rdx_shutdown(void);
const char* rdx_last_error(void);
int         rdx_device_name(char* out, size_t cap);

/* ---- resources: replaces CreateBuffer / CreateImage / ReadBuffer / WriteBuffer
 *      (radiance.h:115-128, radiance.cpp:86-93,139-146,190-204) */
rdx_buffer  rdx_buffer_create(size_t size);
rdx_buffer  rdx_buffer_wrap(void* device_ptr, size_t size);   /* adopt caller-owned device memory (e.g. a torch tensor) */
int         rdx_buffer_write(rdx_buffer b, size_t offset, size_t size, const void* src);
int         rdx_buffer_read(rdx_buffer b, size_t offset, size_t size, void* dst);
void*       rdx_buffer_device_ptr(rdx_buffer b);
size_t      rdx_buffer_size(rdx_buffer b);

/* ---- texture arrays and samplers: replaces CreateImageArray / CreateSampler / ReadImage / WriteImage
 *      (radiance.h:117-124, radiance.cpp:96-137,202-224).  An image array is `layers` RGBA8 images of width x height
 *      (CL_RGBA / CL_UNSIGNED_INT8, layer-major, rows tightly packed); it is also a buffer (rdx_buffer_read/write see the raw
 *      bytes).  write / read move the (width, height) top-left region of one layer, host rows tightly packed, like the
 *      reference's clEnqueue{Write,Read}Image(origin (0,0,layer), region (width,height,1)).  addressingMode / filterMode take
 *      the CL_ADDRESS_* / CL_FILTER_* values the reference's RD_ADDRESS_* / RD_FILTER_* macros expand to.  Bound to descriptor
 *      slots 11 and 12; sampled by the stock closest-hit shader only when option "textures" is 1 (see rdx_set_option).  A user
 *      shader program (rdx_shader_module_create) reads them whatever that option says, through read_imageui(image2d_array_t,
 *      sampler_t, float4), read_imageui(image2d_array_t, int4) and get_image_width / height / array_size / dim, in the
 *      megakernel and in stage mode, with the stock shader's sampler.  A NULL slot 11 reads as an empty image (reads 0,
 *      queries 0), a NULL slot 12 as no sampler (sampled reads 0).  Other image builtins (write_image*, read_imagef /
 *      read_imagei, inline `const sampler_t` constants) would need a hardware image descriptor: such a program is refused at
 *      module creation, naming the builtin. */
rdx_buffer  rdx_image_array_create(uint32_t width, uint32_t height, uint32_t layers);
int         rdx_image_write(rdx_buffer imageArray, uint32_t width, uint32_t height, size_t layer, const void* rgba8);
int         rdx_image_read(rdx_buffer imageArray, uint32_t width, uint32_t height, size_t layer, void* rgba8);
rdx_sampler rdx_sampler_create(uint32_t addressingMode, uint32_t filterMode);

/* ---- acceleration structures: replaces both RD::BuildAccelStruct overloads,
 *      TopAccelStructToFile and FileToTopAccelStruct
 *      (radiance.h:88-92, radiance.cpp:20-84,318-479, radiance/src/bvh.cpp:46-597).
 *      The blobs are byte-identical to the reference's (layout: radiance/shader/data.cl:237-278). */
rdx_blas    rdx_blas_build(const float* vertices_xyz, uint32_t nvertices,
                           const uint32_t* indices, uint32_t ntriangles);
/* `count` meshes at once, built on a pool of host threads inside the library (the caller stays single-threaded);
 * out[i] is what rdx_blas_build(verts[i], ...) would return.  The reference builds its meshes one after the other
 * (tools/sceneBuilder.cpp:229-258); at 10 M triangles that serial loop is the whole scene-load time. */
int         rdx_blas_build_many(uint32_t count, const float* const* verts_xyz, const uint32_t* nvertices,
                                const uint32_t* const* indices, const uint32_t* ntriangles, rdx_blas* out);
const void* rdx_blas_data(rdx_blas b, uint32_t* size_out);
int         rdx_blas_max_depth(rdx_blas b);
rdx_buffer  rdx_tlas_build(const rdx_instance* instances, uint32_t ninstances);
/* Other transforms, SBT offsets or custom ids for the instances of a TLAS that rdx_tlas_build made: afterwards `tlas` holds exactly
 * the blob rdx_tlas_build(instances, ninstances) would have produced -- rdx_buffer_read / rdx_buffer_size / rdx_tlas_to_file return it,
 * every later trace, query, batch and user program sees it.  The handle stays valid and stays bound in descriptor sets; the raw device
 * pointer (rdx_buffer_device_ptr) MAY CHANGE: when the number of top-level nodes changes, the blob's size does, and it moves to a new
 * allocation (the old one is freed: no device memory is lost per call).  Only the top part of the blob is built and uploaded; a
 * traversal layout already derived from the buffer is updated in place -- small arrays, one kernel for the triangles' owner words --
 * or, where the change reaches further (the unified tree or the quad records appear or vanish), derived again in full.
 * Blocks like every call.  Refused, with nothing touched: an uninitialised library, a NULL or unknown handle, a buffer that is not a
 * TLAS built by rdx_tlas_build (rdx_buffer_wrap, rdx_tlas_from_file, plain buffers; a TLAS written to through rdx_buffer_write), an
 * `ninstances` other than the build's, another BLAS handle at any index. */
typedef struct rdx_tlas_update_stats {
    uint32_t path;                 /* 0 = blob only (no layout had been derived yet), 1 = incremental, 2 = full re-derivation */
    uint32_t top_nodes_before, top_nodes_after;
    uint64_t bytes_h2d, bytes_d2d; /* moved by this call, all devices summed */
    uint64_t tri_slots_rewritten;  /* DTri owner words written by the device kernel */
    float    ms_host, ms_device;
} rdx_tlas_update_stats;
int         rdx_tlas_update(rdx_buffer tlas, const rdx_instance* instances, uint32_t ninstances);
int         rdx_get_tlas_update_stats(rdx_tlas_update_stats* out);   /* of the last successful rdx_tlas_update */
/* host-only variant: returns the malloc'ed TLAS blob (release with rdx_free); needs no GPU */
void*       rdx_tlas_build_blob(const rdx_instance* instances, uint32_t ninstances, uint32_t* size_out,
                                int* max_depth_out);
void        rdx_free(void* p);
/* The cache file is the raw blob, as the reference writes it; rdx_tlas_to_file also writes `<path>.meta` (magic,
 * version, byte count, FNV-1a hash) and rdx_tlas_from_file refuses a blob that contradicts an existing side-car. */
int         rdx_tlas_to_file(rdx_buffer tlas, const char* path);
rdx_buffer  rdx_tlas_from_file(const char* path);

/* ---- scene ingestion: replaces the assimp import of RD::Scene::Load (tools/sceneBuilder.cpp:27-258) for Wavefront
 *      OBJ + MTL files: the concatenated vertex / index / uv / normal streams, one MeshInfo per mesh, the Material
 *      table (core.h:122-158 layouts).  Host only, needs no GPU.  Every mesh is one instance (identity transform,
 *      customInstanceID = materialIndex, sceneBuilder.cpp:287-315).  Arrays are malloc'ed; release with rdx_obj_free. */
typedef struct rdx_material {        /* RD::Material, core.h:122-136 / pbr.cl:387-425 (48 B) */
    float   albedo[4];
    float   metallic, roughness, transmission, ior;
    int32_t albedoTexIdx, metallicTexIdx, roughnessTexIdx, normalTexIdx;
} rdx_material;
typedef struct rdx_mesh_info {       /* RD::MeshInfo, core.h:138-148 (32 B); offsets in floats / indices */
    int32_t vertexOffset, indexOffset, uvOffset, normalOffset, materialIndex, _0, _1, _2;
} rdx_mesh_info;
typedef struct rdx_obj_scene {
    uint32_t nmeshes, nvertices, ntriangles, nmaterials;
    rdx_mesh_info* meshInfo;          /* [nmeshes] */
    float*    vertex;                 /* [nvertices][3] */
    uint32_t* index;                  /* [ntriangles][3], mesh-local vertex numbers */
    float*    uv;                     /* [nvertices][3] (u, v, 0) */
    float*    normal;                 /* [nvertices][3] */
    rdx_material* materials;          /* [nmaterials] */
    uint32_t* meshVertexCount;        /* [nmeshes] */
    uint32_t* meshTriangleCount;      /* [nmeshes] */
} rdx_obj_scene;
int         rdx_obj_load(const char* path, rdx_obj_scene* out);
void        rdx_obj_free(rdx_obj_scene* scene);

/* ---- pipeline: replaces CreateShaderModule / BindPipeline / BindDescriptorSet / TraceRays
 *      (radiance.h:130-144, radiance.cpp:152-179,226-267).
 *      `code` is the user's shader text.  The reference's stock program (samples/shader.cl: the stage functions named in
 *      samples/sbt.json -- raygen, material, shadow, anyShadow, environment, shadowMiss) is recognised and served by the
 *      hand-written HIP wavefront pipeline of this library (tools/genSBT.py emits the dispatch); so is a placeholder whose
 *      `raygen` takes no parameters.  ANY OTHER program is compiled at run time by ROCm's OpenCL C compiler for the GPU in
 *      use and launched as a megakernel, one work-item per pixel, parameters bound by position (slots 11 / 12 as null
 *      descriptors) -- as the reference's clBuildProgram + clEnqueueNDRangeKernel would, csrc/user_shader.cpp.  A text that
 *      names no `raygen` kernel, or does not compile (the build log is in rdx_last_error), fails here. */
rdx_shader  rdx_shader_module_create(const char* code, uint32_t size, const char* name);
/* -I directory for `#include "radiance.cl"` etc. in user shader programs: the reference bakes SHADER_LIB_PATH into its
 * binary (radiance.h:7, radiance.cpp:165-167); here it is a run-time setting (the RD:: facade passes SHADER_LIB_PATH). */
int         rdx_shader_include_path(const char* path);
int         rdx_bind_pipeline(rdx_shader raygen_module);
/* handles[i] binds to parameter i of the raygen kernel (samples/shader.cl:175-190):
 * 0 RTProp, 1 imageScratch, 2 image, 3 camData, 4 scene, 5 meshInfo, 6 vertex, 7 index, 8 uv,
 * 9 normal, 10 material, 11 textureArray (may be NULL), 12 sampler (may be NULL), 13 TLAS.  A user program's image2d_array_t /
 * sampler_t parameters receive the library's views of slots 11 / 12 (never a null descriptor; a NULL slot is an empty view). */
int         rdx_bind_descriptor_set(void* const* handles, uint32_t n);
/* the three SBT indices are accepted and ignored, exactly like radiance.cpp:242-259 */
int         rdx_trace_rays(uint32_t raygenGroupIndex, uint32_t missGroupIndex, uint32_t hitGroupIndex,
                           uint32_t width, uint32_t height);

/* ---- extensions (no reference counterpart) ------------------------------------------------ */

/* Image-tile sharding for multi-GPU: this process renders only the pixels whose tile id
 * (row-major over tile_w x tile_h tiles) is congruent to `rank` mod `world`.  Pixel/RNG indices
 * stay global, so the union over ranks is bit-identical to an unsharded frame. */
int         rdx_set_shard(uint32_t rank, uint32_t world, uint32_t tile_w, uint32_t tile_h);
/* pack this rank's tiles of a W*H image of `elem_size`-byte pixels into a contiguous buffer
 * (and the inverse on the gathering rank) */
int         rdx_pack_tiles(rdx_buffer image, rdx_buffer packed, uint32_t width, uint32_t height,
                           uint32_t elem_size, uint32_t rank, uint32_t world);
int         rdx_unpack_tiles(rdx_buffer packed, rdx_buffer image, uint32_t width, uint32_t height,
                             uint32_t elem_size, uint32_t rank, uint32_t world);
/* the same for the packed buffers of ranks first_rank .. first_rank + n - 1 in one call (one synchronisation) */
int         rdx_unpack_tiles_multi(const rdx_buffer* packed, uint32_t first_rank, uint32_t n, rdx_buffer image,
                                   uint32_t width, uint32_t height, uint32_t elem_size, uint32_t world);
uint32_t    rdx_shard_pixel_count(uint32_t width, uint32_t height, uint32_t rank, uint32_t world);

/* Statistics of the last rdx_trace_rays call. */
typedef struct rdx_trace_stats {
    uint64_t rays_primary, rays_bounce, rays_shadow;   /* rays actually traced */
    uint64_t closest_hits;                             /* `material` invocations */
    uint64_t pixels;                                   /* pixels rendered by this rank */
    /* visit counters of the reference algorithm's exhaustive walk, filled only when option
     * "count_visits" is 1: index 0 = radiance rays, 1 = shadow rays (SURVEY.md 8d byte model) */
    uint64_t visit_top_nodes[2], visit_instances[2], visit_bot_nodes[2], visit_triangles[2];
    float    ms_total;                                 /* HIP-event time of the whole call */
    float    ms_generate, ms_extend, ms_shade, ms_shadow, ms_accumulate, ms_fused;  /* ms_fused: shadow(d)+extend(d+1) launches */
    float    ms_path;                                  /* whole-path launches ("pipeline" 1) */
    uint32_t launches_extend, launches_shadow;
    uint32_t groups;                                   /* sample groups the last chunk was traced in (option "groups") */
    float    ms_sort;                                  /* per-bounce ray sort launches (option "sort") */
} rdx_trace_stats;
int         rdx_get_trace_stats(rdx_trace_stats* out);
/* per-bounce visit counters of the last frame traced with "count_visits": out[8*d + 4*c + k], c = 0
 * radiance / 1 shadow rays of bounce d, k = top nodes, instance visits, bottom nodes, triangle tests;
 * returns the number of bounces written (<= max_bounces) */
int         rdx_get_visit_profile(uint64_t* out, uint32_t max_bounces);
/* out[d] = closest-hit rays traced at bounce d of the last frame; out[d+1] is also the number of hits,
 * i.e. of shadow rays, of bounce d */
int         rdx_get_bounce_counts(uint64_t* out, uint32_t n);
/* 0 = per-stage HIP events off (default), 1 = on (adds launch gaps; for profiling only) */
int         rdx_set_profiling(int on);
/* knobs: "chunk_paths" (paths in flight per chunk), "count_visits" (0/1: also count node /
 * triangle visits; slower, for the roofline byte model), "kernel" (traversal kernel: 3 = wave-
 * cooperative with a shared node pool (default), 2 = wave-cooperative with per-lane node stacks, 1 = per-lane wide
 * nodes, 0 = reference order; all four give identical results, the option exists for A/B measurements and
 * cross-checks), "user_shader_local_size" (work-group size of a user shader program's launch, default 64; the reference
 * launches with 1, radiance.cpp:250-259 -- results do not depend on it), "sort" (-1 (default) = automatic: on for scenes of >= 1 M inner BVH nodes, and from 32 k inner nodes on in chunks of more than 1.5 M paths; 1 / 0 = on / off: per-bounce ray sort -- the survivors of a bounce are handed to the
 * traversal launch in (Morton cell of the origin, direction octant) order, by an index permutation from a counting sort; the
 * path streams are not moved and no result depends on it), "textures" (0 (default) / 1.  The live reference shader has every texture read commented out (`uint4 tex =
 * 0.0f;//read_imageui(...)`, samples/shader.cl:379,411,421,445), so a material with a texture index renders with texel 0; that
 * is what 0 reproduces, bit for bit.  1 performs the commented-out read -- coord (uv.x, 1 - uv.y, texIdx), as the reference's
 * older shader2.cl:255-265 does live -- from the image array in slot 11 through the sampler in slot 12.  The option concerns the
 * stock shader only: a user program's own read_imageui calls always read slots 11 / 12), "cull" (pool kernel: -1 (default) = automatic, 1 / 0 = on / off: closest-hit rays skip subtrees the ray enters
 * beyond the best t found so far, every ray skips leaves whose box it misses -- only where a per-node normal cone proves the
 * reference's fp32 intersection test well conditioned for that ray, with margins that cover its error: the result is the
 * reference's exhaustive walk's, docs/CULLED_WALK.md has the proof; automatic = on for scenes with at least 1 M inner BVH
 * nodes, where it pays), "quad" (1 (default) / 0 / -1: the exhaustive walk of the pool engine pops 128-byte quad records -- two levels of the
 * reference's tree per item; 0 = the 64-byte records; -1 = quad records only for chunks of at most 3 M paths;
 * results do not depend on it), "gpu_build" (1 (default) / 0: the BVH builder bins the candidate planes of large nodes on the GPU, DESIGN.md 7.1;
 * "gpu_build_min": nodes and meshes of at least this many primitives, default 32768; blobs do not depend on either),
 * "user_stages" (1 (default) = a user program that equals the stock program outside the bodies of its closest-hit / miss
 * stage functions runs those functions on the wavefront pipeline; 0 = every user program is a megakernel; 2 = the
 * caller asserts eligibility for a program written from scratch, whose raygen is then ignored.  Read by
 * rdx_shader_module_create), "group_instances" (1 (default) / 0: instances whose inverse matrices are bit-identical share one
 * object-space ray and are walked concurrently, traverse_pool.h), "group_entry_items" (1 (default) / 0: over quad records a ray
 * enters all pending instances of that group in one step, as pool items that point at per-instance entry records -- the root
 * test is the pool step's; 0 = one instance record and one root test per instance step; results do not depend
 * on it), "top_flat" (1 (default) / 0: the pool kernel evaluates a top-level tree of <= 64 nodes all at once per
 * ray instead of walking it), "inline_leaf_roots" (1 (default) / 0: ... and tests the triangles of single-leaf BLASes
 * right there), "pipeline" (0 = staged
 * wavefront: one launch per stage per bounce; 1 = whole paths -- camera ray to path end -- in one persistent launch per
 * sample chunk, the closest-hit shader called from the traversal waves; -1 (default) = automatic), "fuse" (1 / -1 = on (default), 0 = off:
 * trace the shadow rays of bounce d and the extend rays of bounce d+1 in one cooperative launch, which
 * halves the fixed ramp + tail cost per bounce), "groups" (0 (default) = automatic, 1..4: the samples of a chunk are
 * traced as that many independent groups on their own streams, each launching its share of the persistent grid, so
 * that one group's launches fill the ramp and drain of the others'; automatic = 2 for chunks of <= 4.7 M paths with
 * at least 2 samples (shards of a multi-GPU frame, low resolutions), else 1; results do not depend on it), "overlap"
 * (experimental: shadow rays on a second stream when "fuse" is 0; off by default) */
int         rdx_set_option(const char* name, int64_t value);

/* Ray queries on device memory: `n` rays of the caller's own, read from `rays` at byte `rays_offset`, against `tlas`; one record
 * per ray written to `hits` at byte `hits_offset`.  Both are device buffers (rdx_buffer_create, or rdx_buffer_wrap around e.g. a
 * torch tensor): nothing is staged through the host and nothing is allocated per call; the call blocks like every call of this ABI
 * (work the caller has queued on streams of its own must be complete before).  Every ray carries its OWN interval: a candidate
 * at distance t is accepted iff t > 0 && t > tmin && t < tmax, the reference's rule (radiance.cl:90-91) with the ray's bounds -- a
 * NaN bound accepts nothing; the shadow ray towards a point light has tmax = the distance to it, an ambient-occlusion ray its
 * radius.  RDX_QUERY_CLOSEST is the walk of traceRay() with sbtRecordOffset 1: on a hit, t / b1 / b2 are the bits of
 * HitData.distance / barycentric[1] / barycentric[2] and the four integers the HitData fields of the same name (hitPoint is
 * origin + t * direction in the instance's space, barycentric[0] is 1 - b1 - b2, the transform is the instance's: all the
 * caller's to derive).  RDX_QUERY_ANY is the walk of sbtRecordOffset 2, which ends at the first accepted candidate, whichever it
 * is: only `hit` is meaningful.  On a miss, and for RDX_QUERY_ANY, every field but `hit` is 0.
 * The engine is chosen as for rdx_trace_batch mode 0, by options "kernel", "cull", "quad", "group_instances", "unified_tree",
 * "top_flat" and "inline_leaf_roots": the pool engine (kernel 3) in a variant that keeps each ray's interval in LDS next to the
 * ray; kernel 2 is served by the per-lane wide-node kernel of kernel 1, as are scenes the pool engine does not
 * fit; kernel 0 and scenes with instance SBT offsets by the reference-order kernel.  Results do not depend on any of them.
 * rdx_get_trace_stats().ms_extend is the kernel time of the call; multi-device mode runs the query on logical device 0.
 * Refused, before anything is launched: an uninitialised library, an unknown or NULL handle, a `kind` other than 1 / 2, an offset
 * that is not a multiple of 16, offset + 32 * n beyond the buffer's size, a ray range that overlaps the hit range.  n == 0
 * succeeds and touches nothing. */
typedef struct rdx_ray     { float origin[3]; float tmin; float direction[3]; float tmax; } rdx_ray;       /* 32 B, two float4 */
typedef struct rdx_ray_hit { float t, b1, b2; uint32_t hit;
                             uint32_t primitiveIndex, instanceIndex, instanceCustomIndex, instanceSBTOffset; } rdx_ray_hit; /* 32 B */
#define RDX_QUERY_CLOSEST 1   /* the walk of sbtRecordOffset 1: the reference's closest hit */
#define RDX_QUERY_ANY     2   /* the walk of sbtRecordOffset 2: only `hit` is meaningful */
int         rdx_query_rays(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, uint32_t n, int kind,
                           rdx_buffer hits, size_t hits_offset);

/* Surface records for the hits of a ray query, on the device: what secondary work needs beyond the ids of an rdx_ray_hit -- the
 * world-space hit point, the surface normal, the origins of the next ray on either side of the surface, the uv and the material
 * number.  `rays` / `hits` are the buffers of an rdx_query_rays(..., RDX_QUERY_CLOSEST, ...) call (record i belongs to ray i;
 * records the caller filled in are equally allowed), `scene` the buffers bound to descriptor slots 5, 7, 8, 9; one 64-byte
 * rdx_surface per ray goes to `out` at byte `out_offset`.  For a hit (`hit` == 1) every field holds the bits the reference's
 * closest-hit shader computes for that HitData under the floating-point contract of DESIGN.md 2: hitPoint = inv (o, 1) +
 * inv (d, 0) * t with the instance's inverse as the traversal layout holds it, barycentric = ((1 - b1) - b2, b1, b2), MeshInfo taken
 * by instanceIndex, normal = getFaceNormal (samples/shader.cl:338-367), above / below = getHitPosition(hitData, +-normal)
 * (shader.cl:453-468: the stock shader's nextRayOrigin is one of the two), (u, v) = getUV (shader.cl:322-336).  Every other record
 * -- a miss, any other value of `hit` -- is 64 zero bytes.  Shading normals from normal maps and material parameters are not
 * resolved here (rdx_shade_hits runs the stock closest-hit shader on the same records).
 * No record makes the kernel read outside a buffer: a hit is INVALID when instanceIndex is not below the TLAS's instance count and
 * the number of MeshInfo records, or one of its three index reads, nine normal reads or six uv reads falls outside its buffer
 * (MeshInfo offsets are int32 and may be negative; the positions are computed in 64 bits), or no instance of the TLAS carries that
 * instanceIndex.  An invalid hit writes the zero record and is counted; the call still returns 0 and *invalid_out (optional)
 * receives the count.  Nothing is staged and nothing is allocated per call; the call blocks like every call of this ABI, accepts
 * every TLAS buffer rdx_query_rays accepts, derives the traversal layout if none exists yet, sees the transforms of the last
 * rdx_tlas_update, and runs on logical device 0 in multi-device mode.  rdx_get_trace_stats().ms_shade is the kernel time of the
 * call.  Refused, before anything is launched: an uninitialised library, an unknown or NULL handle, `scene` NULL or meshInfo /
 * index / normal NULL in it, an offset that is not a multiple of 16, offset + 32 * n (rays, hits) or offset + 64 * n (out) beyond
 * its buffer, `out` overlapping the ray range or the hit range.  n == 0 succeeds and touches nothing. */
typedef struct rdx_surface_buffers { rdx_buffer meshInfo, index, uv, normal; } rdx_surface_buffers;
    /* the buffers of descriptor slots 5, 7, 8, 9; uv may be NULL (u = v = 0) */
typedef struct rdx_surface {                    /* 64 B, four float4 */
    float position[3]; uint32_t hit;            /* HitData.transform * (HitData.hitPoint, 1), xyz; hit: 1 / 0 */
    float normal[3];   uint32_t materialIndex;  /* getFaceNormal (samples/shader.cl:338-367); MeshInfo.materialIndex */
    float above[3];    float u;                 /* getHitPosition(hitData,  normal) (shader.cl:453-468); getUV().x */
    float below[3];    float v;                 /* getHitPosition(hitData, -normal);                     getUV().y */
} rdx_surface;
int         rdx_resolve_hits(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer hits, size_t hits_offset,
                             uint32_t n, const rdx_surface_buffers* scene, rdx_buffer out, size_t out_offset,
                             uint32_t* invalid_out /* optional */);
/* Test seam: the bounds rule above for one record, on the host (needs no device and no initialised library) -> 1 = may be
 * resolved, 0 = invalid.  mi = the MeshInfo records (nmeshinfo of them; read only if instanceIndex is inside), idx3 = the
 * triangle's three vertex numbers (NULL: the rule ends after the index range, which is what must hold before they may be read),
 * nindex / nnormal / nuv = elements of the three streams, nuv == 0: no uv stream, nothing of it is checked. */
int         rdx_debug_surface_in_bounds(const rdx_mesh_info* mi, uint32_t ninst, uint32_t nmeshinfo, uint32_t instanceIndex,
                                        uint32_t primitiveIndex, const uint32_t idx3[3], uint64_t nindex, uint64_t nnormal,
                                        uint64_t nuv);

/* The stock closest-hit shader on the hits of a ray query, on the device: what rdx_trace_rays does between two traversal stages,
 * for the caller's own rays.  `rays` / `hits` are the buffers of an rdx_query_rays(..., RDX_QUERY_CLOSEST, ...) call (record i
 * belongs to ray i; records the caller filled in are equally allowed), `keys` one rdx_shade_key per ray, `scene` the buffers
 * bound to descriptor slots 4, 5, 7, 8, 9, 10, 11, 12.  One 48-byte rdx_shade per ray goes to `shade`.
 * Record with hit == 1: the closest-hit row of the library's shader binding table runs, dispatched as the frame path dispatches
 * it (row instanceSBTOffset + 1; samples/sbt.json: `material`, samples/shader.cl:482-541), on the HitData rdx_resolve_hits derives
 * (hitPoint = inv (o, 1) + inv (d, 0) * t, barycentric = ((1 - b1) - b2, b1, b2), transform by instanceIndex), with rayDir = the
 * ray's direction and (frameID, pixel, depth) of the key as the input of the next direction's random numbers.  The shader traces
 * its shadow ray in the middle of the function; here both outcomes are handed back: `color` is payload.color if the shadow ray
 * is NOT occluded, `colorOccluded` if it is, `nextFactor` is payload.nextFactor -- all with the bits the frame path computes.  The
 * ray SURVIVES and gets a record number k: next[k] = (payload.nextRayOrigin | 0.001, payload.nextRayDirection | 1000), shadow[k]
 * = (the shadow ray's origin | 0.001, normalize(-lights[0].direction) | 1000) -- both ready for rdx_query_rays with the reference's
 * interval -- src[k] = i and shade[i].slot = k.  What the shader of the row does not write keeps the payload's state on entry,
 * which is the frame path's: nextFactor 1, the next ray = the ray itself, no shadow query (a shadow record of zeros: tmax 0
 * accepts nothing, so `color` is chosen) -- so `next` NULL, with which the next direction is not sampled (the last bounce),
 * leaves nextFactor 1.  Any other record: the miss row 3 runs (`environment`: colour (0.2, 0.2, 0.5) in both colour fields), hit = 0, nextFactor
 * = 0, slot = 0xffffffff; the ray does not survive.
 * Without `src`, k = i and record i of a ray that does not survive is 32 zero bytes in `next` / `shadow` (tmax = 0: such a ray
 * accepts nothing).  With `src`, the survivors are packed into records 0 .. live - 1: the survivors among input rays 64 j .. 64 j
 * + 63 occupy consecutive records in input order; the order of these groups among each other is unspecified and may differ from
 * call to call; records from `live` on are left untouched.  *live_out (optional) receives the survivor count either way.
 * Textures follow the stock shader's rule: texels are read, through `sampler` (NULL: repeat, nearest), only when option
 * "textures" is 1 and `textureArray` is given -- `uv` is required then; otherwise a material with a texture index sees texel 0.
 * No record makes the kernel read outside a buffer: a hit is INVALID when rdx_resolve_hits would call it invalid (the uv stream
 * counting only when texels are read), when 3 * primitiveIndex + 2 or 3 * vertex + 2 does not fit 32 bits, when its
 * MeshInfo.materialIndex is not below the number of Material records, or -- texels read -- when one of the Material's four texture
 * indices is neither -1 nor below the layer count.  An invalid hit writes 48 zero bytes except slot = 0xffffffff, does not
 * survive and is counted in *invalid_out (optional); the call still returns 0.
 * Nothing is staged and nothing is allocated per call; the call blocks, derives the traversal layout if none exists yet, sees
 * the transforms of the last rdx_tlas_update, and runs on logical device 0 in multi-device mode.  rdx_get_trace_stats().ms_shade
 * is the kernel time of the call.  Refused, before anything is launched: an uninitialised library; a NULL or unknown handle among
 * tlas / rays / hits / keys / shade / scene / scene->scene, meshInfo, index, normal, material, an unknown one among the optional
 * ones; a scene buffer smaller than a SceneProperties; an offset that is not a multiple of 16; a range that does not hold n
 * records (32 n for rays / hits / next / shadow, 16 n for keys, 48 n for shade, 4 n for src: the worst case); an output range
 * that overlaps an input range or another output range; wrapped memory that is misaligned.  n == 0 succeeds and touches nothing. */
typedef struct rdx_shade_key { uint32_t frameID, pixel, depth, _0; } rdx_shade_key;   /* 16 B: the RNG input pcg3d(frameID, pixel, depth), shader.cl:205 */
typedef struct rdx_shade {                      /* 48 B, three float4 */
    float color[3];         uint32_t hit;           /* payload.color if the shadow ray is NOT occluded; 1 = closest-hit ran, 0 = miss shader ran */
    float colorOccluded[3]; uint32_t materialIndex; /* payload.color if it is occluded */
    float nextFactor[3];    uint32_t slot;          /* record number of this ray's next / shadow ray in `next` / `shadow`, 0xffffffff = none */
} rdx_shade;
typedef struct rdx_shading_buffers { rdx_buffer scene, meshInfo, index, uv, normal, material, textureArray; rdx_sampler sampler; } rdx_shading_buffers;
    /* descriptor slots 4, 5, 7, 8, 9, 10, 11, 12; uv / textureArray / sampler may be NULL */
int         rdx_shade_hits(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer hits, size_t hits_offset,
                           rdx_buffer keys, size_t keys_offset, uint32_t n, const rdx_shading_buffers* scene,
                           rdx_buffer shade, size_t shade_offset,
                           rdx_buffer next, size_t next_offset,        /* optional: rdx_ray per surviving ray */
                           rdx_buffer shadow, size_t shadow_offset,    /* optional: rdx_ray per surviving ray */
                           rdx_buffer src, size_t src_offset,          /* optional uint32 per survivor: switches compaction on */
                           uint32_t* live_out, uint32_t* invalid_out); /* both optional */
/* Test seam: the bounds rule above for one record, on the host (needs no device and no initialised library) -> 1 = may be shaded,
 * 0 = invalid.  Arguments up to nuv as rdx_debug_surface_in_bounds (nuv is ignored unless `textures`); materials = the Material
 * records (nmaterials of them; read only if `textures` and the materialIndex is inside), textures = 1: texels are read, layers =
 * layers of the image array. */
int         rdx_debug_shade_in_bounds(const rdx_mesh_info* mi, uint32_t ninst, uint32_t nmeshinfo, uint32_t instanceIndex,
                                      uint32_t primitiveIndex, const uint32_t idx3[3], uint64_t nindex, uint64_t nnormal,
                                      uint64_t nuv, const rdx_material* materials, uint32_t nmaterials, int textures,
                                      uint32_t layers);

/* The evaluated material of the hits of a ray query, and one directional light's direct term on it, on the device: the two halves
 * of the stock closest-hit shader `material` (samples/shader.cl:482-541) before its next-direction sample, for a caller with a
 * light loop, a BRDF or a denoiser of its own.
 * rdx_resolve_materials: `tlas`, `rays`, `hits`, `scene` are exactly those of rdx_shade_hits (no keys: nothing random is drawn);
 * one 64-byte rdx_material_record per ray goes to `out`.  Record with hit == 1: the HitData is derived as for rdx_shade_hits, and
 * every field holds the bits `material` holds in the variable of the same meaning under the floating-point contract of DESIGN.md
 * 2: normal = N = getMatNormal(..., faceN) (shader.cl:369-395: the face normal, or -- a material with a normal map -- the mapped
 * normal), albedo = getAlbedo (shader.cl:432-451), metallic / roughness / transmission / ior = getMaterialProp (shader.cl:398-430)
 * with its clamps, above = getHitPosition(hitData, faceN) (the origin of the shadow ray), materialIndex = MeshInfo.materialIndex.
 * Textures follow the stock shader's rule as in rdx_shade_hits: texels are read, through `sampler`, only when option "textures" is
 * 1 and `textureArray` is given -- `uv` is required then; otherwise a material with a texture index sees texel 0, the normal map
 * included (whose texel-0 normal is NOT the face normal).  Every other record -- a miss, any other value of `hit` -- is 64 zero
 * bytes.  No record makes the kernel read outside a buffer: the bounds rule is that of rdx_shade_hits, unchanged; a hit it calls
 * INVALID writes the zero record and is counted in *invalid_out (optional), and the call still returns 0.  Staging, blocking,
 * layout derivation on first use, the transforms of the last rdx_tlas_update, logical device 0 in multi-device mode and
 * rdx_get_trace_stats().ms_shade (the kernel time of the call): as for rdx_shade_hits.  Refused, before anything is launched: what
 * rdx_shade_hits refuses, for tlas / rays / hits / out / scene (32 n bytes for rays / hits, 64 n for out; `out` overlapping the
 * ray range or the hit range).  n == 0 succeeds and touches nothing.
 * rdx_light_hits: for light j = `light` of the SceneProperties in `scene` (the buffer of descriptor slot 4; read on the device by
 * every call) and a material record with hit == 1:  L = normalize(-lights[j].direction.xyz), V = normalize(-ray.direction),
 * lit.rgb = (0, 0, 0) + microfacetBRDF(L, V, N, albedo, metallic, roughness, transmission) * lights[j].color.rgb (pbr.cl:268-287),
 * operation for operation the `direct` of `material` (shader.cl:503-508), which it is bit for bit for j = 0; lit.w = 0.  The
 * shadow record (optional) is (above | 0.001, L | 1000), ready for rdx_query_rays(..., RDX_QUERY_ANY, ...): the light reaches the
 * hit iff that query reports no hit.  Any other value of `hit` gives 16 / 32 zero bytes (tmax 0 accepts nothing).  The ambient
 * term stays the caller's (the stock shader's: albedo * 0.1f, once per hit), and lightCount is not consulted, as the stock shader
 * does not consult it.  Only the direction of a ray is read.  The kernel gathers nothing but the one light, so no record can make
 * it read outside a buffer; material records the caller filled in itself are equally allowed.  It takes no TLAS; it blocks, and
 * rdx_get_trace_stats().ms_shade is the kernel time of the call.  Refused, before anything is launched: an uninitialised library;
 * a NULL or unknown handle among rays / materials / scene / lit, an unknown `shadow`; light > 4; a scene buffer smaller than a
 * SceneProperties; an offset that is not a multiple of 16; a range that does not hold n records (32 n for rays / shadow, 64 n for
 * materials, 16 n for lit); an output range that overlaps an input range, the SceneProperties or the other output range; wrapped
 * memory that is misaligned.  n == 0 succeeds and touches nothing. */
typedef struct rdx_material_record {            /* 64 B, four float4 */
    float normal[3];  uint32_t hit;             /* N = getMatNormal(..., faceN) (shader.cl:369-395); hit: 1 / 0 */
    float albedo[3];  uint32_t materialIndex;   /* getAlbedo (shader.cl:432-451); MeshInfo.materialIndex */
    float metallic, roughness, transmission, ior;   /* getMaterialProp (shader.cl:398-430), clamps included */
    float above[3];   uint32_t _0;              /* getHitPosition(hitData, faceN): the shadow ray's origin; _0 = 0 */
} rdx_material_record;
int         rdx_resolve_materials(rdx_buffer tlas, rdx_buffer rays, size_t rays_offset, rdx_buffer hits, size_t hits_offset,
                                  uint32_t n, const rdx_shading_buffers* scene, rdx_buffer out, size_t out_offset,
                                  uint32_t* invalid_out /* optional */);
int         rdx_light_hits(rdx_buffer rays, size_t rays_offset,            /* rdx_ray per record: only the direction is read */
                           rdx_buffer materials, size_t materials_offset,  /* rdx_material_record per ray */
                           uint32_t n, rdx_buffer scene /* slot 4: SceneProperties */, uint32_t light /* 0 .. 4 */,
                           rdx_buffer lit, size_t lit_offset,              /* out float4 per ray: rgb, w = 0 */
                           rdx_buffer shadow, size_t shadow_offset);       /* optional out: rdx_ray per ray */

/* The next ray of the hits of a ray query, on the device: the second half of the stock closest-hit shader `material`
 * (samples/shader.cl:482-541) -- the next-direction sample sampleMicrofacetBRDF_transm (pbr.cl:289-385), nextFactor and the choice
 * between the two offset origins -- on the records of rdx_resolve_materials and rdx_resolve_hits.  With rdx_light_hits it closes
 * the set: a path tracer over any number of lights runs on rdx_query_rays, rdx_resolve_hits, rdx_resolve_materials, rdx_light_hits
 * and this call alone, on the device throughout.
 * A material record with hit == 1:  V = normalize(-ray.direction), N = record.normal, rnd = pcg3d(frameID, pixel, depth) of the key
 * (math.cl:10-23) -- or randoms[i].xyz as they are, for a caller with a sampler of its own; nf = (0, 0, 0); nd =
 * sampleMicrofacetBRDF_transm(V, N, albedo, metallic, roughness, transmission, ior, rnd, &nf); origin = surfaces[i].below if
 * dot(nd, N) < 0, else materials[i].above -- operation for operation what `material` does after its light term (shader.cl:518-540),
 * so on the records of a hit whose SBT row is `material` (instanceSBTOffset 0) nextFactor and the next ray carry the bits of
 * rdx_shade_hits and of the frame path.  The ray SURVIVES and gets a record number k: next[k] = (origin | 0.001, nd | 1000), ready
 * for rdx_query_rays with the reference's interval, scatter[i] = (nf, k), src[k] = i.  Any other value of `hit`: scatter[i] =
 * (0, 0, 0, 0xffffffff), and the ray does not survive.
 * Compaction is that of rdx_shade_hits: without `src`, k = i and record i of a ray that does not survive is 32 zero bytes in `next`
 * (tmax = 0: such a ray accepts nothing).  With `src`, the survivors are packed into records 0 .. live - 1: the survivors among
 * input rays 64 j .. 64 j + 63 occupy consecutive records in input order; the order of these groups among each other is
 * unspecified and may differ from call to call; records from `live` on are left untouched.  *live_out (optional) receives the
 * survivor count either way.
 * Of a ray only the direction is read, of a surface record only `below`.  The kernel gathers nothing, so no record can make it read
 * outside a buffer; records the caller filled in itself are equally allowed.  It takes no TLAS and no scene buffers.  Nothing is
 * staged and nothing is allocated per call; the call blocks, and runs on logical device 0 in multi-device mode.
 * rdx_get_trace_stats().ms_shade is the kernel time of the call.  Refused, before anything is launched: an uninitialised library;
 * a NULL or unknown handle among rays / materials / surfaces / scatter / next, an unknown one among keys / randoms / src; keys and
 * randoms both NULL or both given; an offset that is not a multiple of 16 (4 for src); a range that does not hold n records (32 n
 * for rays / next, 64 n for materials / surfaces, 16 n for keys / randoms / scatter, 4 n for src: the worst case); an output range
 * that overlaps an input range or another output range; wrapped memory that is misaligned.  n == 0 succeeds and touches nothing. */
typedef struct rdx_scatter { float nextFactor[3]; uint32_t slot; } rdx_scatter;   /* 16 B: payload.nextFactor | record number of the next ray in `next`, 0xffffffff = none */
int         rdx_scatter_hits(rdx_buffer rays, size_t rays_offset,            /* rdx_ray per record: only the direction is read */
                             rdx_buffer materials, size_t materials_offset,  /* rdx_material_record per ray */
                             rdx_buffer surfaces, size_t surfaces_offset,    /* rdx_surface per ray: only `below` is read */
                             rdx_buffer keys, size_t keys_offset,            /* rdx_shade_key per ray, or NULL when `randoms` is given */
                             rdx_buffer randoms, size_t randoms_offset,      /* optional float4 per ray: xyz take the place of pcg3d(key), w ignored */
                             uint32_t n,
                             rdx_buffer scatter, size_t scatter_offset,      /* out: rdx_scatter per ray */
                             rdx_buffer next, size_t next_offset,            /* out: rdx_ray per surviving ray */
                             rdx_buffer src, size_t src_offset,              /* optional uint32 per survivor: switches compaction on */
                             uint32_t* live_out);                            /* optional */

/* The two ends of a frame, on the device: the camera rays a loop over rdx_query_rays / rdx_shade_hits starts from, and the step
 * that folds its finished samples into the frame rdx_trace_rays would have written.
 * rdx_generate_rays: ray i is generateRay (samples/shader.cl:111-173) for pixel_i = pixels ? pixels[i] : first_pixel + i, with
 * the random input pcg3d(seed_i) (math.cl:10-23), seed_i = seeds ? seeds[i].in : (frameID, totalSamples, pixel_i) -- the three
 * inputs of shader.cl:205, where frameID = totalSamples + the sample's number in the batch.  Origin and direction carry the bits
 * the frame path's own generate stage computes under the floating-point contract of DESIGN.md 2, thin lens (fStop != 0)
 * included; tmin / tmax are written into every ray as passed (the reference's are 0.001f / 1000.0f): the records are ready for
 * rdx_query_rays.  `keys` (optional) receives the rdx_shade_key {frameID, pixel_i, 0, 0} of every ray: the key of depth 0 for
 * rdx_shade_hits.  `camera` holds a PhysicalCamera -- the contents of descriptor slot 3; it need not be bound -- and is read on
 * the device by every call: cos / sin of its angles are evaluated there, per call, by the OCML functions the reference links, so
 * a camera written between two calls is seen by the second.  A pixel number only enters arithmetic; none is refused.
 * rdx_accumulate: sample i, colors[i] (float4: rgb, w ignored), belongs to pixel_i as above and is sample `frameID` of that
 * pixel's running mean in `scratch` (imageScratch, slot 1: float4 per pixel): rgb = colour when frameID == 0, otherwise
 * (float(frameID) * rgb + colour) / float(frameID + 1), the reference's expression (shader.cl:262-270) operation for operation;
 * w stays as it is.  `image` (optional; slot 2: RGBA8) receives that pixel's (unsigned char)(int)(c * 255) | 255 of c =
 * pow(ACES(mean), 0.7f) (shader.cl:272-304), or of c = mean with flags bit 0 (RTProp.debug).  One call is one frameID: the
 * samples of a batch are a loop of calls, in sample order.  The frame has min(size(scratch) / 16, size(image) / 4) pixels; a
 * pixel number not below that writes nothing and is counted in *invalid_out (optional), and the call still returns 0.  The
 * pixels of one call must be distinct: for a pixel named twice the result is that of ONE of its samples, unspecified which
 * (never an access outside the buffers).
 * Both: device memory in and out (rdx_buffer_create, or rdx_buffer_wrap around e.g. a torch tensor), nothing staged through the
 * host, nothing allocated per call; the call blocks, and runs on logical device 0 in multi-device mode.
 * rdx_get_trace_stats().ms_generate / .ms_accumulate is the kernel time of the call (for rdx_generate_rays including the one
 * thread that prepares the camera).  Refused, before anything is launched: an uninitialised library; a NULL or unknown camera /
 * rays / colors / scratch handle, an unknown one among the optional ones; a camera buffer smaller than a PhysicalCamera; an
 * offset that is not a multiple of 16 (4 for `pixels`); a range that does not hold n records (32 n rays, 16 n keys / seeds /
 * colors, 4 n pixels); first_pixel + n beyond 2^32 when `pixels` is NULL; an output range (rays, keys; the whole of scratch and
 * image) that overlaps an input range or the other output range; flags other than bit 0; wrapped memory that is misaligned.
 * n == 0 succeeds and touches nothing. */
typedef struct rdx_raygen_seed { uint32_t in[3]; uint32_t _0; } rdx_raygen_seed;   /* 16 B: the three inputs of pcg3d (shader.cl:205) */
int         rdx_generate_rays(rdx_buffer camera,                       /* a PhysicalCamera (descriptor slot 3 contents); need not be bound */
                              uint32_t n, uint32_t first_pixel,
                              rdx_buffer pixels, size_t pixels_offset, /* optional uint32 per ray; NULL: ray i is pixel first_pixel + i */
                              uint32_t frameID, uint32_t totalSamples,
                              rdx_buffer seeds, size_t seeds_offset,   /* optional rdx_raygen_seed per ray; NULL: (frameID, totalSamples, pixel) */
                              float tmin, float tmax,                  /* written into every ray; the reference's are 0.001f / 1000.0f */
                              rdx_buffer rays, size_t rays_offset,     /* out: rdx_ray per ray */
                              rdx_buffer keys, size_t keys_offset);    /* optional out: rdx_shade_key {frameID, pixel, 0, 0} per ray */
#define RDX_ACCUMULATE_DEBUG 1u   /* flags bit 0: RTProp.debug (skip ACES and gamma) */
int         rdx_accumulate(rdx_buffer colors, size_t colors_offset,   /* float4 per sample: rgb, w ignored */
                           uint32_t n, uint32_t first_pixel,
                           rdx_buffer pixels, size_t pixels_offset,   /* optional uint32 per sample; NULL: first_pixel + i */
                           uint32_t frameID,
                           rdx_buffer scratch,                        /* imageScratch: float4 per pixel (slot 1) */
                           rdx_buffer image,                          /* optional RGBA8 (slot 2): NULL = no tone map */
                           uint32_t flags,                            /* bit 0: RTProp.debug (skip ACES and gamma) */
                           uint32_t* invalid_out);                    /* optional */

/* Radiance along the caller's own rays, on the device: the whole raygen loop between rdx_generate_rays and rdx_accumulate in one
 * call, on the frame path's own stages -- the fused shadow + extend launch, the per-bounce ray sort, ballot compaction -- for
 * rays of any origin: another camera model, light probes, lightmap texels, irradiance caches.  Path i starts with ray i and key i
 * (frameID and pixel; `depth` and `_0` are ignored): radiance[i].rgb is the value of `color` at the end of the reference's raygen
 * `while` loop (samples/shader.cl:231-260) entered with payload.nextRayOrigin / nextRayDirection = ray i, sceneData.frameID =
 * keys[i].frameID, get_global_id(0) = keys[i].pixel, depth 0 and RTProp.depth = max_depth; radiance[i].w is 0.  The rows of the
 * library's shader binding table are dispatched as the frame path dispatches them, colour and contribution are folded operation
 * for operation as the frame path's shade and shadow stages fold them (color += contribution * payload.color, contribution *=
 * payload.nextFactor; a primary miss shows the miss colour, a later miss ends the path), so for the rays and keys of
 * rdx_generate_rays the result is the sample rdx_accumulate expects -- generate -> trace_paths -> accumulate writes the frame
 * rdx_trace_rays writes -- and it has the bits of the loop over rdx_query_rays / rdx_shade_hits shown in the README.  (One
 * difference from that loop, in scenes with instance SBT offsets only: a shadow ray that meets an instance dispatches row
 * instanceSBTOffset + 2 here as in the frame path and the reference, and a row without a hit shader does not occlude; the loop's
 * RDX_QUERY_ANY reports `hit` alone.)  The first traceRay uses
 * ray i's OWN interval under the rule of rdx_query_rays (a NaN bound accepts nothing); every later segment and every shadow query
 * the reference's 0.001 / 1000.  Directions need not be unit length.  max_depth == 0 gives zeros.  `hits` (optional) receives the
 * first segment's records: exactly what rdx_query_rays(tlas, rays, ..., RDX_QUERY_CLOSEST, hits, ...) writes.  User stage
 * programs do not run here (as for rdx_shade_hits); only lights[0] is sampled, as by the stock shader.
 * TRUST: `scene` (descriptor slots 4, 5, 7, 8, 9, 10, 11, 12 as for rdx_shade_hits, textures by the same rule: option "textures" 1
 * and a textureArray, uv required then) must describe the scene of `tlas`.  Every hit comes from the library's own traversal of
 * `tlas`, so the shade stage gathers UNCHECKED, exactly as in rdx_trace_rays -- unlike rdx_shade_hits, which shades records of
 * any origin and fences every gather.  The one record format the caller can reach, the first segment's in `hits`, is still
 * mapped to a miss when its instanceIndex is not below the TLAS's instance count or no instance carries it.
 * Options "kernel", "cull", "quad", "sort", "fuse", "group_instances", "group_entry_items", "unified_tree", "top_flat" and
 * "inline_leaf_roots" apply as in rdx_trace_rays (the first segment: as in rdx_query_rays); no result depends on them.
 * "pipeline", "groups", "overlap" and "count_visits" do not apply: one group of paths, staged.  More than "chunk_paths" paths are
 * traced in chunks of that many.  Nothing is staged through the host; the path streams (and, without `hits`, one chunk of
 * records) grow on first use as rdx_trace_rays' do and are reused.  The call blocks, derives the traversal layout if none exists
 * yet, sees the transforms of the last rdx_tlas_update, and runs on logical device 0 in multi-device mode.  rdx_get_trace_stats
 * (pixels = n, ray counts, launches, ms_total; with rdx_set_profiling the ms_* of the stages: ms_extend includes the first
 * segment, ms_generate is the kernel that turns rays into paths) and rdx_get_bounce_counts are filled as by rdx_trace_rays.
 * Refused, before anything is launched: an uninitialised library; a NULL or unknown handle among tlas / rays / keys / radiance /
 * scene / scene->scene, meshInfo, index, normal, material, an unknown one among the optional ones; a scene buffer smaller than a
 * SceneProperties; max_depth > 62; an offset that is not a multiple of 16; a range that does not hold n records (32 n for rays /
 * hits, 16 n for keys / radiance); an output range (radiance, hits) that overlaps an input range or the other output range;
 * wrapped memory that is misaligned.  n == 0 succeeds and touches nothing; records from n on are never written. */
int         rdx_trace_paths(rdx_buffer tlas,
                            rdx_buffer rays, size_t rays_offset,          /* rdx_ray per path: the first segment, with ITS tmin / tmax */
                            rdx_buffer keys, size_t keys_offset,          /* rdx_shade_key per path: frameID, pixel (depth, _0 ignored) */
                            uint32_t n, uint32_t max_depth,               /* RTProp.depth; 0 .. 62 */
                            const rdx_shading_buffers* scene,             /* slots 4, 5, 7, 8, 9, 10, 11, 12 as for rdx_shade_hits */
                            rdx_buffer radiance, size_t radiance_offset,  /* out: float4 per path: rgb, w = 0 */
                            rdx_buffer hits, size_t hits_offset);         /* optional out: rdx_ray_hit of the first segment */

/* Radiance along `n` rays of the caller's own with EVERY directional light of the scene sampled at every hit -- the reference's
 * closest-hit shader ends its light term with "TODO: support multiple lights" (samples/shader.cl:504) and reads lights[0] only, as
 * do rdx_trace_rays, rdx_shade_hits and rdx_trace_paths.  Rays and keys as for rdx_trace_paths; light_count (0 .. 5) lights,
 * lights[0 .. light_count - 1] of the SceneProperties in scene->scene, are read ON THE DEVICE by every call (SceneProperties.
 * lightCount is not consulted, as no other call consults it).  radiance[i].rgb is `color` of the path tracer over the public calls
 * shown in the README (its second loop), bit for bit, run on ray i, key i, max_depth and light_count; radiance[i].w is 0.  Each
 * float32 operation is rounded on its own.  Per live ray at depth d:
 *   query   a closest-hit query under the ray's own interval (the rule of rdx_query_rays): the first segment carries the caller's
 *           tmin / tmax, every later one the 0.001 / 1000 of rdx_scatter_hits;
 *   miss    a record whose `hit` is not 1, or a hit the bounds rule rejects (below): at depth 0 the colour becomes the stock miss
 *           colour (0.2, 0.2, 0.5); at a later depth the path ends with the colour it has;
 *   hit     the material record is that of rdx_resolve_materials, `below` that of rdx_resolve_hits; direct = (0, 0, 0); for j = 0 ..
 *           light_count - 1 in this order: lit_j and its shadow ray are those of rdx_light_hits for light j, the shadow ray is
 *           answered by an RDX_QUERY_ANY query, direct = direct + (occluded ? 0 : lit_j); radiance = direct + albedo * 0.1f;
 *           color = color + weight * radiance; weight = weight * nextFactor, with nextFactor and the next ray those of
 *           rdx_scatter_hits under the key (frameID, pixel, d).
 * max_depth == 0 gives zeros; at the last depth no next ray is sampled or traced (no result depends on it).  light_count == 0 is
 * valid and leaves the ambient term.  Two consequences:
 *   - for light_count == 1 the result has the bits of rdx_trace_paths, and of the frames rdx_trace_rays writes (generate ->
 *     trace_paths_lights(1) -> accumulate), in scenes without instance SBT offsets;
 *   - with instance SBT offsets the call follows the README's loop: RDX_QUERY_ANY reports `hit` alone, so a shadow ray that meets
 *     an instance whose row instanceSBTOffset + 2 has no hit shader still occludes.  That is the difference rdx_trace_paths
 *     documents, from the other side.
 * FENCED: unlike rdx_trace_paths this call gathers checked.  Every hit passes the bounds rule of rdx_shade_hits / rdx_resolve_
 * materials (csrc/shade.h shade_in_bounds, asked before and after the index gather) and must name an instance the TLAS carries, so
 * `scene` buffers that do not describe the scene of `tlas` cannot make a kernel read outside a buffer: such a hit is a miss and is
 * counted in *invalid_out (optional).  Textures follow the rule of rdx_shade_hits (option "textures" 1 and a textureArray; uv
 * required then).  User closest-hit programs do not run here; lights with a position are rdx_trace_paths_punctual's, area lights
 * rdx_trace_paths_area's (both below); one device.
 * Nothing is staged through the host: the library reads back ONE 32-bit word per bounce, the survivors' count that sizes the next
 * launches.  Internal streams of 192 + 80 light_count bytes per path of a chunk grow on first use and are reused.  More than
 * "chunk_paths" paths are traced in chunks of that many.  The call blocks, derives the traversal layout if none exists yet, sees
 * the transforms of the last rdx_tlas_update, and runs on logical device 0 in multi-device mode.  The engine options ("kernel",
 * "cull", "quad", "group_instances", "group_entry_items", "unified_tree", "top_flat", "inline_leaf_roots") apply as in
 * rdx_query_rays; no result depends on them.  rdx_get_trace_stats: pixels = n, rays_primary = n, rays_bounce = the live rays of the
 * depths >= 1, closest_hits = the valid hits, rays_shadow = light_count x closest_hits, launches_extend / launches_shadow = the
 * closest-hit / any-hit launches, ms_total; with rdx_set_profiling ms_extend / ms_shadow = those launches and ms_shade = the two
 * kernels of this call.  rdx_get_bounce_counts: out[0] = n, out[d + 1] = the survivors of depth d.
 * Refused, before anything is launched: everything rdx_trace_paths refuses (`hits` aside); light_count > 5; max_depth > 62; a
 * radiance range that overlaps the SceneProperties.  n == 0 succeeds and touches nothing; records from n on are never written. */
int         rdx_trace_paths_lights(rdx_buffer tlas,
                                   rdx_buffer rays, size_t rays_offset,          /* rdx_ray per path: the first segment, with ITS tmin / tmax */
                                   rdx_buffer keys, size_t keys_offset,          /* rdx_shade_key per path: frameID, pixel (depth, _0 ignored) */
                                   uint32_t n, uint32_t max_depth,               /* 0 .. 62 */
                                   uint32_t light_count,                         /* 0 .. 5: lights[0 .. light_count - 1] of the SceneProperties */
                                   const rdx_shading_buffers* scene,             /* slots 4, 5, 7, 8, 9, 10, 11, 12 as for rdx_shade_hits */
                                   rdx_buffer radiance, size_t radiance_offset,  /* out: float4 per path: rgb, w = 0 */
                                   uint32_t* invalid_out);                       /* optional */

/* Point and spot lights, from a light TABLE of the caller's own in device memory: records of 64 bytes, each directional, point or
 * spot, read ON THE DEVICE by every call.  Two calls on the two levels of the light API above: rdx_punctual_light_hits is
 * rdx_light_hits for one record of the table, rdx_trace_paths_punctual is rdx_trace_paths_lights over its first light_count
 * records.  Neither changes rdx_light_hits or rdx_trace_paths_lights.
 * rdx_punctual_light_hits: rays, materials, n, lit and shadow are those of rdx_light_hits; the light is the ONE record at byte
 * offset light_offset (index * 64) of `lights`.  For a material record with hit == 1, every float32 operation rounded on its own,
 * with N, V, normalize (v_rsq_f32 based, as everywhere in the library), microfacetBRDF and clamp exactly those of rdx_light_hits:
 *   type 0  L = normalize(-direction), E = color, tmax = 1000.0f: bit for bit rdx_light_hits on a DirLight {direction, color};
 *   type 1, 2  v = position - above (three subtractions); d2 = (v.x * v.x + v.y * v.y) + v.z * v.z (plain products and sums, not
 *           fused); L = normalize(v); att = 1.0f / d2; E = color * att; tmax = sqrtf(d2) -- the shadow ray ends AT the light;
 *   type 2  in addition S = normalize(direction); c = -((S.x * L.x + S.y * L.y) + S.z * L.z); f = clamp(c * coneScale + coneOffset,
 *           0.0f, 1.0f) (a multiplication, then an addition); E = E * (f * f);
 *   DARK    the record is dark at the hit if type > 2; or, types 1 and 2, !(d2 > 0.0f), !(d2 < INFINITY), or range > 0.0f &&
 *           !(d2 < range * range); or, type 2, !(f > 0.0f);
 *   else    lit.rgb = (0, 0, 0) + microfacetBRDF(L, V, N, albedo, metallic, roughness, transmission) * E, lit.w = 0, and the shadow
 *           record (optional) is (above | 0.001f, L | tmax), ready for rdx_query_rays(..., RDX_QUERY_ANY, ...).
 * A dark record and any other value of `hit` give 16 zero bytes in `lit` and 32 in `shadow` (tmax 0 accepts nothing).  The kernel
 * gathers nothing but the one record, so no record can make it read outside a buffer; non-finite fields give unspecified colours,
 * never a fault.  The call blocks; rdx_get_trace_stats().ms_shade is the kernel time.  Refused, before anything is launched: what
 * rdx_light_hits refuses for rays / materials / lit / shadow; a NULL or unknown `lights`; a light_offset that is not a multiple of
 * 16; 64 bytes at light_offset that do not fit `lights`; an output range that overlaps the light.  n == 0 succeeds and touches
 * nothing.
 * rdx_trace_paths_punctual: the per-path specification of rdx_trace_paths_lights, word for word, with "light j of the
 * SceneProperties via rdx_light_hits" read as "record j of the table (at lights_offset + 64 j) via rdx_punctual_light_hits", and
 * the shadow rays carrying that call's tmax: direct = ((0 + x_0) + x_1) + ..., x_j = occluded_j ? 0 : lit_j; a record that is dark
 * at a hit contributes its zero `lit` through a shadow ray that accepts nothing.  radiance[i].rgb is `color` of the README's loop
 * over rdx_punctual_light_hits, bit for bit; with type-0 records alone it has the bits of rdx_trace_paths_lights on the same lights
 * as DirLights.  Fenced gathers, the miss colour at depth 0, one 32-bit word read back per bounce, the engine options, the stats
 * and the bounce counts: as for rdx_trace_paths_lights.  scene->scene is still required (slot 4); its lights are not read.  The
 * internal streams take 192 + 80 light_count bytes per path of a chunk, in the allocation rdx_trace_paths_lights uses; beyond 5
 * records a chunk is min("chunk_paths", "chunk_paths" * 592 / (192 + 80 light_count)) paths, so that the allocation is no larger
 * than that call's worst case; no result depends on chunking.  Refused, before anything is launched: everything
 * rdx_trace_paths_lights refuses (its light_count rule aside); light_count > RDX_MAX_PATH_LIGHTS; a NULL or unknown `lights`; a
 * lights_offset that is not a multiple of 16; 64 light_count bytes at lights_offset that do not fit `lights`; a radiance range
 * that overlaps the table.  n == 0 succeeds and touches nothing. */
#define RDX_LIGHT_DIRECTIONAL 0u
#define RDX_LIGHT_POINT       1u
#define RDX_LIGHT_SPOT        2u
typedef struct rdx_punctual_light {              /* 64 B, four float4 */
    float position[3];  uint32_t type;           /* point / spot: world-space position */
    float direction[3]; float range;             /* the direction the light shines ALONG (as DirLight.direction); range: 0 = unlimited */
    float color[3];     float _0;                /* directional: as DirLight.color; point / spot: the colour at distance 1 */
    float coneScale, coneOffset, _1, _2;         /* spot: 1 / max(0.001, cosInner - cosOuter), -cosOuter * coneScale (the caller computes them) */
} rdx_punctual_light;
#define RDX_MAX_PATH_LIGHTS 16u
int         rdx_punctual_light_hits(rdx_buffer rays, size_t rays_offset,            /* rdx_ray: only the direction is read */
                                    rdx_buffer materials, size_t materials_offset,  /* rdx_material_record per ray */
                                    uint32_t n,
                                    rdx_buffer lights, size_t light_offset,         /* ONE rdx_punctual_light at this byte offset (index * 64) */
                                    rdx_buffer lit, size_t lit_offset,              /* out float4 per ray: rgb, w = 0 */
                                    rdx_buffer shadow, size_t shadow_offset);       /* optional out: rdx_ray per ray */
int         rdx_trace_paths_punctual(rdx_buffer tlas,
                                     rdx_buffer rays, size_t rays_offset,          /* rdx_ray per path: the first segment, with ITS tmin / tmax */
                                     rdx_buffer keys, size_t keys_offset,          /* rdx_shade_key per path: frameID, pixel (depth, _0 ignored) */
                                     uint32_t n, uint32_t max_depth,               /* 0 .. 62 */
                                     rdx_buffer lights, size_t lights_offset,      /* the table: rdx_punctual_light records */
                                     uint32_t light_count,                         /* 0 .. RDX_MAX_PATH_LIGHTS records */
                                     const rdx_shading_buffers* scene,             /* slots 4, 5, 7, 8, 9, 10, 11, 12 as for rdx_shade_hits */
                                     rdx_buffer radiance, size_t radiance_offset,  /* out: float4 per path: rgb, w = 0 */
                                     uint32_t* invalid_out);                       /* optional */

/* Area lights, from a SECOND light table of the caller's own in device memory: records of 64 bytes, each a parallelogram or a
 * triangle that emits a constant radiance, read ON THE DEVICE by every call.  An emitter is sampled at ONE point per (hit, light),
 * uniformly over its area, so its shadows are soft over frames.  Two calls on the two levels of the light API above:
 * rdx_area_light_hits is rdx_punctual_light_hits for one area record, rdx_trace_paths_area is rdx_trace_paths_punctual over a
 * punctual table AND an area table.  Neither changes any other call.
 * The emitters are NOT geometry: a camera ray does not see them, and a path that reaches lamp geometry of the scene shades that
 * geometry's ordinary material.  The estimator is next-event only -- a light is counted where it is sampled, never where a path
 * happens to arrive --, so nothing is counted twice.  No textured or spherical emitters, no multiple-importance sampling, one
 * sample per light per hit.
 * The emitter is corner + s * edgeU + t * edgeV with s, t in [0, 1] (RDX_AREA_QUAD) or the triangle corner, corner + edgeU, corner +
 * edgeV (RDX_AREA_TRIANGLE).  n = cross(edgeU, edgeV) points away from the emitting face, into the half-space the record lights
 * (edgeU = +x, edgeV = +z: a lamp that shines down); a one-sided record is dark from behind; flags bit 0 (RDX_AREA_TWO_SIDED) makes
 * it emit from both faces.
 * rdx_area_light_hits: rays, materials, n, lit and shadow are those of rdx_punctual_light_hits; the light is the ONE record at byte
 * offset light_offset (index * 64) of `lights`.  Exactly one of `keys` and `randoms` is given, by rdx_scatter_hits' rule: keys are
 * rdx_shade_key records, randoms one float4 per ray of which x and y are used.  For a material record with hit == 1, every float32
 * operation rounded on its own, with N, V, normalize (v_rsq_f32 based), microfacetBRDF and clamp exactly those of rdx_light_hits:
 *   keys     r = pcg3d(key.frameID, key.pixel, key.depth + ((stream + 1u) << 16)) in uint32 arithmetic; u = r.x, v = r.y.  Paths are
 *            at most 62 deep and sample at most 16 records, so no (depth, stream) pair meets the pcg3d(frameID, pixel, depth) that
 *            rdx_scatter_hits draws from, or another stream's;
 *   randoms  u = randoms[i].x, v = randoms[i].y, as they are;
 *   type 1   if (u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
 *   p.c = (corner.c + edgeU.c * u) + edgeV.c * v for c = x, y, z (plain products and sums, not fused);
 *   n.x = edgeU.y * edgeV.z - edgeU.z * edgeV.y; n.y = edgeU.z * edgeV.x - edgeU.x * edgeV.z; n.z = edgeU.x * edgeV.y - edgeU.y * edgeV.x;
 *   w = p - above; d2 = (w.x * w.x + w.y * w.y) + w.z * w.z; L = normalize(w);
 *   g = -((n.x * L.x + n.y * L.y) + n.z * L.z); type 1: g = g * 0.5f; flags bit 0: g = fabsf(g) -- emitter area x cosine at the
 *            emitter: |n| is the parallelogram's area, so nothing is normalised and no square root is taken;
 *   E = radiance * (g / d2): one division, three products -- the one-sample estimator under the pdf 1 / area; microfacetBRDF
 *            carries the receiver's cosine, as for every other light;
 *   tmax = sqrtf(d2) * 0.999f: the shadow ray STOPS SHORT of the emitter, so lamp geometry that lies in the light's own plane --
 *            the quad under a Cornell box's ceiling -- does not shadow its own light (nor does anything else within the last
 *            thousandth of the distance);
 *   DARK     the record is dark at the hit if type > 1, !(d2 > 0.0f), !(d2 < INFINITY) or !(g > 0.0f) -- the back face of a
 *            one-sided record, a degenerate emitter, NaNs;
 *   else     lit.rgb = (0, 0, 0) + microfacetBRDF(L, V, N, albedo, metallic, roughness, transmission) * E, lit.w = 0, and the shadow
 *            record (optional) is (above | 0.001f, L | tmax), ready for rdx_query_rays(..., RDX_QUERY_ANY, ...).
 * A dark record and any other value of `hit` give 16 zero bytes in `lit` and 32 in `shadow`.  The kernel gathers nothing but the
 * one record and the ray's key or randoms; non-finite fields give unspecified colours, never a fault.  The call blocks;
 * rdx_get_trace_stats().ms_shade is the kernel time.  Refused, before anything is launched: what rdx_punctual_light_hits refuses,
 * with the 64 bytes of the area record in the place of the punctual one; both of keys and randoms, or neither; a keys_offset or
 * randoms_offset that is not a multiple of 16, or 16 n bytes there that do not fit; an output range that overlaps the keys or the
 * randoms; stream > 0xfffe.  n == 0 succeeds and touches nothing.
 * rdx_trace_paths_area: the per-path specification of rdx_trace_paths_punctual over BOTH tables.  At every hit the light_count
 * records of `lights` are evaluated first, as that call evaluates them; then the area_count records of `area`, record j via
 * rdx_area_light_hits on the keys route with stream = j and the path's own (frameID, pixel, depth); they are folded in that order:
 * direct = ((0 + x_0) + x_1) + ..., x = occluded ? 0 : lit.  light_count + area_count <= RDX_MAX_PATH_LIGHTS; either count may be
 * 0, and its table may then be NULL.  radiance[i].rgb is `color` of the README's loop over the two per-hit calls, bit for bit; with
 * area_count == 0 it has the bits of rdx_trace_paths_punctual.  Streams, chunking, stats, bounce counts, the one word read back per
 * bounce, the fenced gathers, the miss colour and the engine options: as for rdx_trace_paths_punctual with light_count +
 * area_count in the place of light_count.  Refused, before anything is launched: everything rdx_trace_paths_punctual refuses (a NULL
 * table of no records aside); light_count + area_count > RDX_MAX_PATH_LIGHTS; a NULL or unknown `area` with area_count != 0; an
 * area_offset that is not a multiple of 16; 64 area_count bytes at area_offset that do not fit `area`; a radiance range that
 * overlaps either table.  n == 0 succeeds and touches nothing. */
#define RDX_AREA_QUAD      0u   /* the parallelogram corner + s * edgeU + t * edgeV, s, t in [0, 1] */
#define RDX_AREA_TRIANGLE  1u   /* the triangle corner, corner + edgeU, corner + edgeV */
#define RDX_AREA_TWO_SIDED 1u   /* flags bit 0: emits from both faces */
typedef struct rdx_area_light {                  /* 64 B, four float4 */
    float corner[3];   uint32_t type;
    float edgeU[3];    uint32_t flags;
    float edgeV[3];    float _0;
    float radiance[3]; float _1;                 /* emitted radiance, constant over the emitter */
} rdx_area_light;
int         rdx_area_light_hits(rdx_buffer rays, size_t rays_offset,              /* rdx_ray: only the direction is read */
                                rdx_buffer materials, size_t materials_offset,    /* rdx_material_record per ray */
                                uint32_t n,
                                rdx_buffer lights, size_t light_offset,           /* ONE rdx_area_light at this byte offset (index * 64) */
                                rdx_buffer keys, size_t keys_offset,              /* rdx_shade_key per ray, or NULL */
                                uint32_t stream,                                  /* keys route: 0 .. 0xfffe, the record's random stream */
                                rdx_buffer randoms, size_t randoms_offset,        /* float4 per ray (x, y used), or NULL */
                                rdx_buffer lit, size_t lit_offset,                /* out float4 per ray: rgb, w = 0 */
                                rdx_buffer shadow, size_t shadow_offset);         /* optional out: rdx_ray per ray */
int         rdx_trace_paths_area(rdx_buffer tlas,
                                 rdx_buffer rays, size_t rays_offset,             /* rdx_ray per path: the first segment, with ITS tmin / tmax */
                                 rdx_buffer keys, size_t keys_offset,             /* rdx_shade_key per path: frameID, pixel (depth, _0 ignored) */
                                 uint32_t n, uint32_t max_depth,                  /* 0 .. 62 */
                                 rdx_buffer lights, size_t lights_offset,         /* the table of rdx_punctual_light records */
                                 uint32_t light_count,
                                 rdx_buffer area, size_t area_offset,             /* the table of rdx_area_light records */
                                 uint32_t area_count,                             /* light_count + area_count <= RDX_MAX_PATH_LIGHTS */
                                 const rdx_shading_buffers* scene,                /* slots 4, 5, 7, 8, 9, 10, 11, 12 as for rdx_shade_hits */
                                 rdx_buffer radiance, size_t radiance_offset,     /* out: float4 per path: rgb, w = 0 */
                                 uint32_t* invalid_out);                          /* optional */

/* The environment: a lat-long image of width x height float32 RGBA texels in device memory (alpha ignored), importance-sampled at
 * ONE direction per hit.  Row 0 is the zenith (+y); column x covers the azimuth [2 pi x / W, 2 pi (x + 1) / W); the direction of
 * (theta, phi) is (sin theta cos phi, cos theta, sin theta sin phi).  1 <= width <= 16384, 1 <= height <= 8192.  No rotation or
 * intensity (scale or roll the image), one sample per hit, no multiple-importance sampling, no filtering; user closest-hit
 * programs do not run here; one device.  The reference has no environment light.
 * rdx_env_table_size(width, height): the bytes of the sampling table, 0 for a size outside the limits.
 * rdx_env_build writes the table of the image at image_offset into the caller's buffer at table_offset (both multiples of 16), on
 * the device, in stream order; the call blocks.  The parts are 16-byte aligned (padding is zero), in this order:
 *   header   64 bytes: uint32 magic 0x56454452, version 1, width, height; float32 wmax, twoPiOverW = (float)(2 pi / W), wOverTwoPi =
 *            (float)(W / (2 pi)); uint32 0; uint64 total; 24 zero bytes;
 *   rowCos   float32[H + 1]: (float)cos(pi y / H), computed by the host in double; entry 0 is exactly 1, entry H exactly -1.  Rows
 *            are bands of cos(theta), so a texel's solid angle is twoPiOverW * (rowCos[y] - rowCos[y + 1]) and the device evaluates
 *            no transcendental for the table or for E;
 *   C        uint32[H][W]: the inclusive prefix sums along each row of
 *            w = max(r, max(g, b)) * (rowCos[y] - rowCos[y + 1]) in float32 (a NaN channel makes the maximum a NaN), taken as 0
 *                where it is not finite or not positive; wmax = the maximum of w;
 *            q = 0 where w == 0, else max(1, min(65535, (uint32)(w * (65535.0f / wmax)))): every texel with any light in it can
 *                be sampled;
 *   M        uint64[H]: the inclusive prefix sums of the row sums; total = M[H - 1].
 * Maximum and integer sums do not depend on the order they are taken in: the table's bytes are a function of the image alone.
 * rdx_env_light_hits is rdx_area_light_hits with the environment in the place of the one record: rays, materials, n, keys |
 * randoms, stream, lit and shadow are that call's.  The random triple (u, v, z) is pcg3d(key.frameID, key.pixel, key.depth +
 * ((stream + 1u) << 16)) on the keys route and x, y, z of the caller's float4 on the randoms route; u can be exactly 1.0.  For a
 * material record with hit == 1, every float32 operation rounded on its own:
 *   X = min((uint64)((double)u * (double)total), total - 1)  (a caller's u outside [0, 1] or NaN is held to the two ends);
 *   y = the first row with M[y] > X; lo = y ? M[y - 1] : 0; rowSum = M[y] - lo;
 *   fy = ((float)(X - lo) + 0.5f) / (float)rowSum;
 *   Xc = min((uint64)((double)v * (double)rowSum), rowSum - 1); x = the first column with C[y][x] > Xc;
 *   q = C[y][x] - (x ? C[y][x - 1] : 0); fx = z;
 *   ct = rowCos[y] + fy * (rowCos[y + 1] - rowCos[y]); st = sqrtf(max(0, 1 - ct * ct)); phi = ((float)x + fx) * twoPiOverW;
 *   L = (st * cosf(phi), ct, st * sinf(phi)), not normalised again;
 *   E = image[y][x].rgb * ((((float)total / (float)q) * twoPiOverW) * (rowCos[y] - rowCos[y + 1])): the one-sample estimator under
 *            the pdf q / (total * the texel's solid angle);
 *   tmax = 1000.0f, the stock interval, as for a directional light;
 *   DARK     total == 0; the header's magic, width or height are not the call's; q == 0;
 *   else     lit and the shadow record as for rdx_area_light_hits.
 * A dark record and any other value of `hit` give 16 zero bytes in `lit` and 32 in `shadow`.  Every index formed from table
 * contents is held to [0, H) / [0, W), and both searches are bounded by H and W, not by table contents: a table of garbage gives
 * unspecified colours, never a read outside the image and table ranges.  Refused, before anything is launched: what
 * rdx_area_light_hits refuses, with the image and table ranges -- 16 W H bytes and rdx_env_table_size(W, H) bytes at offsets that
 * are multiples of 16 -- in the place of the area record; a size outside the limits; an output range that overlaps the image or the
 * table.  n == 0 succeeds and touches nothing.
 * rdx_env_lookup: radiance[i] = (rgb, 0) of the texel the environment shows along the direction of ray i, with the texel's bits;
 * zeros for a zero or non-finite direction and for a table whose header is not the call's.  The row is the band of rowCos that
 * holds normalize(d).y -- the first y with rowCos[y + 1] < it, the sampling bands --, the column min((uint32)(phi * wOverTwoPi),
 * W - 1) with phi = atan2f(d.z, d.x), plus 6.2831855f where negative.  Nearest texel, no filtering.
 * rdx_trace_paths_env is rdx_trace_paths_area with the environment as one more record AFTER the light_count punctual and the
 * area_count area records, sampled via rdx_env_light_hits on the keys route with stream = area_count; light_count + area_count + 1
 * <= RDX_MAX_PATH_LIGHTS.  A path whose FIRST ray hits nothing shows rdx_env_lookup of that ray in the place of the stock miss
 * colour; a later miss ends the path and adds nothing: light is counted by next-event estimation alone, so nothing is counted
 * twice.  radiance[i].rgb is `color` of the README's loop over the per-hit calls, bit for bit.  Everything else, the refusals
 * included, as for rdx_trace_paths_area, with the image and table ranges added; the radiance range may overlap neither. */
size_t      rdx_env_table_size(uint32_t width, uint32_t height);
int         rdx_env_build(rdx_buffer image, size_t image_offset,                  /* float4 per texel, row-major, row 0 = +y */
                          uint32_t width, uint32_t height,
                          rdx_buffer table, size_t table_offset);                 /* out: rdx_env_table_size(width, height) bytes */
int         rdx_env_light_hits(rdx_buffer rays, size_t rays_offset,               /* rdx_ray: only the direction is read */
                               rdx_buffer materials, size_t materials_offset,     /* rdx_material_record per ray */
                               uint32_t n,
                               rdx_buffer image, size_t image_offset,
                               rdx_buffer table, size_t table_offset,             /* as rdx_env_build wrote it for this image */
                               uint32_t width, uint32_t height,
                               rdx_buffer keys, size_t keys_offset,               /* rdx_shade_key per ray, or NULL */
                               uint32_t stream,                                   /* keys route: 0 .. 0xfffe */
                               rdx_buffer randoms, size_t randoms_offset,         /* float4 per ray (x, y, z used), or NULL */
                               rdx_buffer lit, size_t lit_offset,                 /* out float4 per ray: rgb, w = 0 */
                               rdx_buffer shadow, size_t shadow_offset);          /* optional out: rdx_ray per ray */
int         rdx_env_lookup(rdx_buffer rays, size_t rays_offset, uint32_t n,       /* rdx_ray: only the direction is read */
                           rdx_buffer image, size_t image_offset,
                           rdx_buffer table, size_t table_offset,
                           uint32_t width, uint32_t height,
                           rdx_buffer radiance, size_t radiance_offset);          /* out float4 per ray: rgb, w = 0 */
int         rdx_trace_paths_env(rdx_buffer tlas,
                                rdx_buffer rays, size_t rays_offset,              /* rdx_ray per path: the first segment, with ITS tmin / tmax */
                                rdx_buffer keys, size_t keys_offset,              /* rdx_shade_key per path: frameID, pixel (depth, _0 ignored) */
                                uint32_t n, uint32_t max_depth,                   /* 0 .. 62 */
                                rdx_buffer lights, size_t lights_offset,          /* the table of rdx_punctual_light records */
                                uint32_t light_count,
                                rdx_buffer area, size_t area_offset,              /* the table of rdx_area_light records */
                                uint32_t area_count,                              /* light_count + area_count + 1 <= RDX_MAX_PATH_LIGHTS */
                                rdx_buffer image, size_t image_offset,
                                rdx_buffer table, size_t table_offset,
                                uint32_t width, uint32_t height,
                                const rdx_shading_buffers* scene,                 /* slots 4, 5, 7, 8, 9, 10, 11, 12 as for rdx_shade_hits */
                                rdx_buffer radiance, size_t radiance_offset,      /* out: float4 per path: rgb, w = 0 */
                                uint32_t* invalid_out);                           /* optional */

/* Multiple-importance sampling of the environment: the direction rdx_env_light_hits draws from the table and the direction
 * rdx_scatter_hits draws from the material are weighted against each other by the balance heuristic, so that a bounce ray that
 * leaves the scene is SEEN: a mirror and a pane of glass show the sky, and a glossy surface under a broad sky converges sooner.
 * Punctual and area records are not geometry and stay pure next-event estimation; area emitters stay invisible.
 * At a hit with material record (N, albedo, metallic, roughness r, transmission, ior) and V = normalize(-ray direction), every
 * float32 operation rounded on its own, dot(a, b) = fma(a.z, b.z, fma(a.y, b.y, a.x * b.x)), normalize as in the reference:
 *   lobe(rnd)     of a scatter sample, from the random triple rdx_scatter_hits drew it with: TRANSMISSION (2) if rnd.z < 0.5f &&
 *                 2.0f * rnd.z < transmission, else DIFFUSE (0) if rnd.z < 0.5f, else SPECULAR (1); NONE (3) for a direction the
 *                 environment's table gave;
 *   pdf_scatter(L) NoL = dot(N, L); 0 unless NoL > 0, else H = normalize(V + L); NoH = clamp(dot(N, H), 0, 1); VoH = clamp(dot(V, H), 0,
 *                 1); a2 = (r * r) * (r * r); den = NoH * NoH * (a2 - 1.0f) + 1.0f; D = a2 / (3.14159265359f * den * den);
 *                 pSpec = D * NoH / (4.0f * VoH); pDiff = min(NoL, 1.0f) / 3.14159265359f; t = clamp(transmission, 0, 1);
 *                 pdf_scatter = 0.5f * pSpec + (0.5f * (1.0f - t)) * pDiff: the density with which the two reflective lobes together
 *                 produce L;
 *   pdf_env(d)    0 where rdx_env_lookup shows nothing (a zero or non-finite d, a header that is not the call's) and where total == 0;
 *                 else, with the row y and the column x of rdx_env_lookup, q = C[y][x] - (x ? C[y][x - 1] : 0) and
 *                 pdf_env = ((float)q / (float)total) / (twoPiOverW * (rowCos[y] - rowCos[y + 1])): the density with which
 *                 rdx_env_light_hits produces d;
 *   w_scatter     1.0f if the lobe is TRANSMISSION, if it is SPECULAR and (r * r) * (r * r) == 0.0f, if !(NoL > 0), if pdf_scatter or
 *                 pdf_env is not finite, or if !(pdf_scatter + pdf_env > 0); else pdf_scatter / (pdf_scatter + pdf_env).
 *   The environment's weight is 1.0f - w_scatter.
 * rdx_env_mis_weights evaluates this for n directions: direction k is dirs[k].direction -- a `shadow` range of rdx_env_light_hits
 * or a `next` range of rdx_scatter_hits, as those calls write them -- seen from ray / material record s = src ? src[k] : k (the
 * `src` of rdx_scatter_hits; without it nrecords must equal n).  keys or randoms are the nrecords rows rdx_scatter_hits was given
 * and give the lobe of record s; with neither, the lobe is NONE.  out[k] is an rdx_env_mis_weight.  16 zero bytes for s >=
 * nrecords, a record whose hit is not 1, a direction of zeros and a row whose tmax is 0 (a dark shadow row, a dead next row).  The
 * kernel gathers through src alone, held to nrecords, and every table index is held to the call's W and H.  Refused, before
 * anything is launched: invalid handles; offsets that are not multiples of 16 (of 4 for src); a range outside its buffer; `out` overlapping any
 * input; both keys and randoms; nrecords != n without src; a size outside the limits.  n == 0 succeeds and touches nothing.
 * rdx_trace_paths_env_mis is rdx_trace_paths_env, same arguments and refusals, with three changes to the README's loop:
 *   the environment's lit of a hit is scaled, lit.rgb * (1.0f - w_scatter(its shadow direction, lobe NONE)), each channel, at
 *   every depth but the last (depth + 1 < max_depth);
 *   w = w_scatter(the next direction, the sample's lobe) is kept with the path after rdx_scatter_hits;
 *   a live ray of depth >= 1 without a valid hit -- a miss, or a hit the scene buffers do not describe -- adds
 *   color += weight * (rdx_env_lookup(ray).rgb * w), weight being the path's after the previous fold.
 * Depth 0 is unchanged (a first miss shows the texel).  The last depth samples no next ray, so no scatter sample would carry the
 * share w_scatter of its hit: there the environment's lit counts in full, as in rdx_trace_paths_env, and the truncated path
 * estimates the same integral as that call's wherever every lobe can be sampled both ways.  Both reflective lobes share
 * w_scatter(L) over the upper hemisphere, so their weighted sum and the weighted next-event term add up to the unweighted BRDF;
 * transmission and the r == 0 mirror are counted by the scatter sample alone.  A transmission sample's total-internal-reflection
 * fallback direction is weighted 1 like the rest of its lobe.  radiance[i].rgb is `color` of that loop, bit for bit. */
#define RDX_LOBE_DIFFUSE 0u
#define RDX_LOBE_SPECULAR 1u
#define RDX_LOBE_TRANSMISSION 2u
#define RDX_LOBE_NONE 3u
typedef struct rdx_env_mis_weight {
    float    w_scatter, pdf_scatter, pdf_env;
    uint32_t lobe;
} rdx_env_mis_weight;
int         rdx_env_mis_weights(rdx_buffer rays, size_t rays_offset,              /* rdx_ray per record: the direction is read -> V */
                                rdx_buffer materials, size_t materials_offset,    /* rdx_material_record per record */
                                rdx_buffer dirs, size_t dirs_offset, uint32_t n,  /* rdx_ray per direction: the direction and tmax are read */
                                rdx_buffer src, size_t src_offset,                /* optional uint32 per direction: its record; NULL: k */
                                uint32_t nrecords,                                /* rows of rays / materials / keys / randoms */
                                rdx_buffer keys, size_t keys_offset,              /* rdx_shade_key per record, or NULL */
                                rdx_buffer randoms, size_t randoms_offset,        /* float4 per record (z used), or NULL; both NULL: lobe NONE */
                                rdx_buffer image, size_t image_offset,
                                rdx_buffer table, size_t table_offset,
                                uint32_t width, uint32_t height,
                                rdx_buffer out, size_t out_offset);               /* out: rdx_env_mis_weight per direction */
int         rdx_trace_paths_env_mis(rdx_buffer tlas,
                                    rdx_buffer rays, size_t rays_offset,          /* as rdx_trace_paths_env, every argument */
                                    rdx_buffer keys, size_t keys_offset,
                                    uint32_t n, uint32_t max_depth,
                                    rdx_buffer lights, size_t lights_offset,
                                    uint32_t light_count,
                                    rdx_buffer area, size_t area_offset,
                                    uint32_t area_count,
                                    rdx_buffer image, size_t image_offset,
                                    rdx_buffer table, size_t table_offset,
                                    uint32_t width, uint32_t height,
                                    const rdx_shading_buffers* scene,
                                    rdx_buffer radiance, size_t radiance_offset,
                                    uint32_t* invalid_out);

/* The frame's denoiser, on the device: an edge-avoiding a-trous wavelet filter (Dammertz et al. 2010) over a width x height image
 * of float4 colours -- what rdx_trace_paths and its kin write for the rays of rdx_generate_rays, pixel p = y * width + x -- guided
 * by the rdx_material_record and the rdx_surface of the same pixels' primary hits (records the caller filled in are equally
 * allowed).  valid(p) = materials[p].hit == 1 && surfaces[p].hit == 1; n = materials[p].normal, a = materials[p].albedo, P =
 * surfaces[p].position.  Every float32 operation below is rounded on its own; dot is fma(z, z', fma(y, y', x x')).
 * Prepare: den_k = DEMODULATE ? fmaxf(a_k, 0.015625f) : 1 (a NaN albedo gives 0.015625); i_0(p)_k = valid ? color[p]_k / den_k :
 * color[p]_k.
 * Pass j = 0 .. passes - 1, s = 1 << j, h = {1/16, 1/4, 3/8, 1/4, 1/16}: an invalid p keeps its iterate.  For a valid p, sum = 0,
 * sumw = 0, and for dy = -2 .. 2, inside that dx = -2 .. 2, q = (x + dx s, y + dy s), skipped when outside the image or not valid:
 *     k  = h[dy + 2] * h[dx + 2]
 *     wn = fmaxf(dot(n(p), n(q)), 0), squared normal_squarings times
 *     wz = sigma_position == 0 ? 1 : fmaxf(1 - fabsf(dot(n(p), P(q) - P(p))) / (sigma_position * (float)s), 0)
 *     l(c) = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b of the current iterate; x = fabsf(l(p) - l(q)) / (sigma_colour * 2^-j)
 *     wc = sigma_colour == 0 ? 1 : 1 / (1 + x * x)
 *     w  = ((k * wn) * wz) * wc; the tap is skipped unless w > 0 and the three components of i_j(q) are finite
 *     sum_k = sum_k + i_j(q)_k * w; sumw = sumw + w
 * i_{j+1}(p) = sumw > 0 ? sum / sumw (one division per component) : i_j(p).
 * Finish: out[p].rgb = valid ? i_passes(p)_k * den_k : color[p].rgb; out[p].w = color[p].w, its bits kept; image[p] (optional,
 * RGBA8) is the tone map of rdx_accumulate on out[p].rgb, with RDX_DENOISE_DEBUG as its debug bit.  passes == 0 is prepare and
 * finish alone.  A pixel's result depends on this order of taps only, not on how the work is cut into launches and blocks.
 * `work` is rdx_denoise_work_size(width, height) bytes of the caller's (0 for a size outside 1 .. 16384 x 1 .. 16384 or above
 * 2^26 pixels; at most 64 bytes per pixel); its contents before and after a call are unspecified.  Nothing is staged and nothing
 * is allocated per call; the call blocks and runs on logical device 0 in multi-device mode.  rdx_get_trace_stats().ms_accumulate
 * is the kernel time of the call.  Refused, before anything is launched: an uninitialised library; a NULL or unknown handle among
 * color / materials / surfaces / work / out, an unknown `image`; `settings` NULL, passes > 8, normal_squarings > 7, a sigma that
 * is negative, infinite or a NaN, non-zero padding, unknown flag bits; a size outside the limits; an offset that is not a
 * multiple of 16 (4 for `image`); a range that does not hold width x height records (16 per pixel for color / out, 64 for
 * materials / surfaces, 4 for image, the work size); `work`, `out` or `image` overlapping an input range or each other; wrapped
 * memory that is misaligned.  width == 0 or height == 0 succeeds and touches nothing.
 * Not covered: a variance guide (rdx_temporal_accumulate below accumulates over frames and estimates the variance;
 * rdx_svgf_filter further below is this filter with that variance as its guide), guides beyond the primary hit (a reflection is
 * filtered as the surface it appears on); sigma_position is in the caller's world units. */
#define RDX_DENOISE_DEMODULATE 1u   /* divide by the clamped albedo before the passes, multiply it back after them */
#define RDX_DENOISE_DEBUG      2u   /* the tone map's RTProp.debug: no ACES, no gamma */
typedef struct rdx_denoise_settings {      /* 32 B */
    uint32_t passes;             /* 0 .. 8: pass j uses step 1 << j; 0 copies */
    uint32_t normal_squarings;   /* 0 .. 7: normal weight = max(n.n', 0) squared this many times (5 -> power 32) */
    float    sigma_position;     /* world units of plane distance at step 1; 0 = term off; otherwise finite and > 0 */
    float    sigma_colour;       /* luminance units at pass 0, halved every pass; 0 = term off; otherwise finite and > 0 */
    uint32_t flags;              /* bit 0 RDX_DENOISE_DEMODULATE, bit 1 RDX_DENOISE_DEBUG (tone map: RTProp.debug) */
    uint32_t _0[3];              /* must be 0 */
} rdx_denoise_settings;
size_t      rdx_denoise_work_size(uint32_t width, uint32_t height);
int         rdx_denoise(rdx_buffer color, size_t color_offset,           /* float4 per pixel, row-major, rgb + w */
                        rdx_buffer materials, size_t materials_offset,   /* rdx_material_record per pixel */
                        rdx_buffer surfaces, size_t surfaces_offset,     /* rdx_surface per pixel */
                        uint32_t width, uint32_t height, const rdx_denoise_settings* settings,
                        rdx_buffer work, size_t work_offset,             /* rdx_denoise_work_size bytes; contents before and after unspecified */
                        rdx_buffer out, size_t out_offset,               /* float4 per pixel */
                        rdx_buffer image, size_t image_offset);          /* optional RGBA8 per pixel */
/* Test and measurement seam: bit j of `mask` (j = 0, 1: steps 1 and 2) makes that pass of every later rdx_denoise take its taps from
 * an LDS tile of the block's pixels and their halo, a clear bit straight from memory.  Both forms give the same bits; the default
 * is 3, the faster form of both steps. */
void        rdx_debug_denoise_tiled(uint32_t mask);

/* Temporal accumulation, on the device: the temporal half of SVGF (Schied et al. 2017).  A frame's history is carried to the current
 * camera through the previous view, its taps are tested against the history's own guide, and colour and the first two luminance
 * moments are folded into exponential means with a per-pixel variance estimate.  Every float32 operation below is rounded on its
 * own; dot is fma(z, z', fma(y, y', x x')); divisions are IEEE divisions; no transcendental is evaluated per pixel.
 *
 * rdx_camera_view writes the rdx_view of `camera`, the PhysicalCamera buffer exactly as rdx_generate_rays reads it (its current
 * contents, on the device).  With c* = cosf, s* = sinf of wx, wy, wz (the OCML functions of rdx_generate_rays) and the row-major
 *     RotX = {1, 0, 0;  0, cx, -sx;  0, sx, cx}   RotY = {cy, 0, sy;  0, 1, 0;  -sy, 0, cy}   RotZ = {cz, -sz, 0;  sz, cz, 0;  0, 0, 1}
 * M = RotX (RotY RotZ): first T = RotY RotZ, then M = RotX T, every element of a product (a_i0 b_0j + a_i1 b_1j) + a_i2 b_2j.
 * right, up and back are the columns 0, 1, 2 of M (the camera looks along -back); kx = focalLength / sensorWidth; ky =
 * focalLength / (sensorWidth * (heightPixel / widthPixel)).  The record is plain data: a caller with a camera of their own fills
 * it directly.  Refused: an uninitialised library; a NULL or unknown handle; a camera buffer below 48 bytes; view_offset no
 * multiple of 16; a view range that does not hold 64 bytes or overlaps the camera.  rdx_get_trace_stats().ms_generate is its time.
 * The sample-space position of a world point Q under a view V:
 *     v  = Q - V.eye
 *     dz = -dot(V.back, v);                     Q is in front of the camera iff dz > 0
 *     u  = V.width * 0.5f + (V.width * V.kx) * (dot(V.right, v) / dz)
 *     t  = V.height * 0.5f - (V.height * V.ky) * (dot(V.up, v) / dz)
 * the inverse of the ray of rdx_generate_rays for fStop == 0: the point origin + s direction of the ray of pixel (x, y) with jitter
 * rnd lands at u = x + rnd.x, t = y + rnd.y up to rounding.  The thin lens (fStop != 0) is NOT inverted: its rays start on the
 * lens, and a point off the focal plane projects to the centre of its circle of confusion.
 *
 * rdx_temporal_accumulate, per pixel p = y * width + x.  valid(p) = materials[p].hit == 1 && surfaces[p].hit == 1 (the rule of
 * rdx_denoise); n = materials[p].normal, mi = materials[p].materialIndex, P = surfaces[p].position, c = color[p].rgb.
 * A history is four planes of width x height float4, rdx_temporal_history_size(width, height) = 64 width height bytes (0 for a
 * size outside 1 .. 16384 x 1 .. 16384 or above 2^26 pixels):
 *     plane 0  c'.rgb | w: the bits of color[p].w        (rdx_denoise takes it as `color` at the history's offset, without a copy)
 *     plane 1  m1 | m2 | variance | N                    (N: the history length, a uint32)
 *     plane 2  n.xyz | mi
 *     plane 3  P.xyz | valid                             (1u or 0u)
 * 1. An invalid p writes color[p]'s bits to plane 0, zeros and N = 0 to plane 1, n | mi and P | 0 to planes 2 and 3, and is no
 *    one's tap, now or in the next frame.
 * 2. Q = previous_positions ? previous_positions[p].xyz : P: where this surface point was one frame ago.
 * 3. du = u(previous_view, Q) - u(view, P); dt = t(previous_view, Q) - t(view, P); the history position is hx = (float)x + du, hy =
 *    (float)y + dt in texel units.  Sign convention: a camera that moved by one pixel's width along +right finds pixel (x, y)'s
 *    history at (x + 1, y).  Subtracting the current view's own projection removes the sub-pixel jitter; with bit-equal views and
 *    Q = P the motion is exactly +0 and the history position exactly the pixel.
 * 4. x0 = floorf(hx), fx = hx - x0, wx = {1 - fx, fx}; likewise y0, fy, wy.  Taps (x0 + i, y0 + j), j = 0, 1 outer, i = 0, 1 inner,
 *    weight w = wx[i] * wy[j].  A tap q counts iff it lies inside the image, history_in is given, q's valid == 1 and N >= 1, q's mi
 *    equals mi, dot(n, n(q)) >= normal_cos_min, position_tolerance == 0 or fabsf(dot(n, P(q) - Q)) <= position_tolerance, w > 0
 *    and the three components of q's colour are finite (a comparison with a NaN fails).  For a counted tap sum_k = sum_k + h(q)_k * w,
 *    s1 = s1 + m1(q) * w, s2 = s2 + m2(q) * w, sumw = sumw + w, Nh = min(Nh, N(q)).  dz <= 0 under either view, or a du or dt that
 *    is not finite: no tap counts.
 * 5. l = (0.2126f * c.r + 0.7152f * c.g) + 0.0722f * c.b.  With sumw > 0: h = sum / sumw, m1h = s1 / sumw, m2h = s2 / sumw (one
 *    division each); N' = min(Nh + 1, max_history) (no wrap); a = fmaxf(1.0f / (float)N', alpha_min), am = fmaxf(1.0f / (float)N',
 *    alpha_moments_min); c'_k = h_k + (c_k - h_k) * a; m1' = m1h + (l - m1h) * am; m2' = m2h + (l * l - m2h) * am.
 *    Without: N' = 1, c' = c, m1' = l, m2' = l * l.
 *    A c with a component that is not finite: with history c' = h, m1' = m1h, m2' = m2h, N' = Nh (the history is kept as it is);
 *    without, c' = c's bits, m1' = m2' = 0 and N' = 0, so that it is no one's tap.
 * 6. variance = fmaxf(m2' - m1' * m1', 0) where N' >= variance_min_history.  Elsewhere, in a second launch over the new history:
 *    s1 = s2 = sumw = 0, and for dy = -3 .. 3, inside that dx = -3 .. 3, q = (x + dx, y + dy) inside the image with N'(q) >= 1 and
 *    mi(q) == mi: w = fmaxf(dot(n, n(q)), 0), skipped unless w > 0 and w, m1'(q), m2'(q) are finite; s1 = s1 + m1'(q) * w; s2 = s2 +
 *    m2'(q) * w; sumw = sumw + w.  M1 = sumw > 0 ? s1 / sumw : m1', M2 likewise; variance = fmaxf(M2 - M1 * M1, 0) *
 *    ((float)variance_min_history / (float)max(N', 1)): SVGF's boost for young pixels.
 * 7. image[p] (optional, RGBA8) is the tone map of rdx_accumulate on plane 0's rgb, with RDX_TEMPORAL_DEBUG as its debug bit.
 * previous_view NULL is `view`; history_in NULL starts a history (N' = 1 on every valid pixel).  Nothing is staged and nothing is
 * allocated per call; the call blocks and runs on logical device 0 in multi-device mode.  rdx_get_trace_stats().ms_accumulate is
 * the kernel time of the call.  Refused, before anything is launched: an uninitialised library; a NULL or unknown handle among
 * color / materials / surfaces / view / history_out, an unknown one among the optional four; `settings` NULL, max_history outside
 * 1 .. 65535, alpha_min or alpha_moments_min outside [0, 1] or a NaN, a normal_cos_min that is not finite, a position_tolerance
 * that is negative, infinite or a NaN, variance_min_history above 255, unknown flag bits, non-zero padding; a size outside the
 * limits; an offset that is not a multiple of 16 (4 for `image`); a range that does not hold its records (16 bytes per pixel for
 * color / previous_positions, 64 for materials / surfaces, 64 for a view, the history size, 4 per pixel for image); history_out or
 * image overlapping any input -- history_in included -- or each other; wrapped memory that is misaligned.  width == 0 or height == 0
 * succeeds and touches nothing.
 * Not covered: the variance guide inside rdx_denoise's passes (rdx_svgf_filter below reads plane 1), a wider search when all four taps fail,
 * albedo demodulation of the history (a caller may pass demodulated colours), the thin lens, anything beyond the primary hit. */
#define RDX_TEMPORAL_DEBUG 1u       /* the tone map's RTProp.debug: no ACES, no gamma */
typedef struct rdx_view {                  /* 64 B: four float4 */
    float eye[3],   widthPixel;
    float right[3], heightPixel;
    float up[3],    kx;
    float back[3],  ky;
} rdx_view;
typedef struct rdx_temporal_settings {     /* 32 B */
    uint32_t max_history;            /* 1 .. 65535: N saturates here, so alpha never falls below 1 / max_history */
    float    alpha_min;              /* 0 .. 1: the least weight of the current colour */
    float    alpha_moments_min;      /* 0 .. 1: the same for the two luminance moments */
    float    normal_cos_min;         /* finite: a tap counts if dot(n, n') >= this */
    float    position_tolerance;     /* world units of plane distance; 0 = term off; otherwise finite and > 0 */
    uint32_t variance_min_history;   /* 0 .. 255: below this N the variance is the 7 x 7 spatial estimate (SVGF: 4); 0 = never */
    uint32_t flags;                  /* bit 0 RDX_TEMPORAL_DEBUG */
    uint32_t _0;                     /* must be 0 */
} rdx_temporal_settings;
int         rdx_camera_view(rdx_buffer camera,                                  /* PhysicalCamera, as for rdx_generate_rays */
                            rdx_buffer view, size_t view_offset);               /* out: one rdx_view */
size_t      rdx_temporal_history_size(uint32_t width, uint32_t height);
int         rdx_temporal_accumulate(rdx_buffer color, size_t color_offset,                         /* float4 per pixel, row-major, rgb + w */
                                    rdx_buffer materials, size_t materials_offset,                 /* rdx_material_record per pixel */
                                    rdx_buffer surfaces, size_t surfaces_offset,                   /* rdx_surface per pixel */
                                    rdx_buffer previous_positions, size_t previous_positions_offset,   /* optional float4 per pixel */
                                    rdx_buffer view, size_t view_offset,                           /* rdx_view */
                                    rdx_buffer previous_view, size_t previous_view_offset,         /* optional rdx_view; NULL = view */
                                    uint32_t width, uint32_t height, const rdx_temporal_settings* settings,
                                    rdx_buffer history_in, size_t history_in_offset,               /* optional: the previous frame's history_out */
                                    rdx_buffer history_out, size_t history_out_offset,             /* rdx_temporal_history_size bytes */
                                    rdx_buffer image, size_t image_offset);                        /* optional RGBA8 per pixel */

/* The variance-guided a-trous filter of SVGF (Schied et al. 2017), on the device: the passes of rdx_denoise with a luminance weight
 * that is normalised by the local standard deviation -- wide where the estimate is noisy, narrow where a history has converged --
 * and with the variance filtered along by the squared weights.  `color` is typically plane 0 of a history of
 * rdx_temporal_accumulate and `moments` its plane 1, both taken at the history's offsets without a copy; of moments[p] only .z, the
 * variance, is read.  Every float32 operation below is rounded on its own; dot is fma(z, z', fma(y, y', x x')); divisions are IEEE
 * divisions and sqrtf is the correctly rounded one; no transcendental is evaluated per pixel.
 * valid, n, a, P, den_k, l(c), h, k, wn and wz are those of rdx_denoise, word for word.
 * Prepare: ld = DEMODULATE ? l(den) : 1 (the luminance formula on the three den_k); i_0(p)_k = valid ? color[p]_k / den_k :
 * color[p]_k; vz = moments[p].z;
 *     v_0(p) = (valid && vz > 0 && vz < inf) ? vz / (ld * ld) : 0
 * so that a NaN, a negative or an infinite variance counts as 0.
 * Pass j = 0 .. passes - 1, s = 1 << j: an invalid p keeps i_j(p) and v_j(p).  For a valid p, first the 3 x 3 prefilter of the
 * variance, always at distance 1 whatever s is: g = {1/4, 1/2, 1/4}, gs = 0, gw = 0, and for dy = -1 .. 1, inside that dx = -1 .. 1,
 * q = (x + dx, y + dy), skipped when outside the image or not valid (the centre always counts):
 *     gs = gs + (g[dy + 1] * g[dx + 1]) * v_j(q); gw = gw + g[dy + 1] * g[dx + 1]
 *     gv = gs / gw; sd = sqrtf(gv); dl = sigma_luminance * sd + epsilon
 * (with sigma_luminance == 0 nothing reads dl).  Then sum = 0, sv = 0, sumw = 0 and the 25 taps in the order of rdx_denoise, dy =
 * -2 .. 2, inside that dx = -2 .. 2, q = (x + dx s, y + dy s), skipped when outside the image or not valid, k, wn and wz unchanged:
 *     x  = fabsf(l(i_j(p)) - l(i_j(q))) / dl
 *     wc = sigma_luminance == 0 ? 1 : 1 / (1 + x * x)
 *     w  = ((k * wn) * wz) * wc; the tap is skipped unless w > 0, the three components of i_j(q) are finite and v_j(q) is finite
 *     sum_k = sum_k + i_j(q)_k * w; sv = sv + v_j(q) * (w * w); sumw = sumw + w
 * With sumw > 0: i_{j+1}(p) = sum / sumw (one division per component) and v_{j+1}(p) = sv / (sumw * sumw); otherwise both are kept.
 * (With sigma_luminance == 0 this is rdx_denoise with sigma_colour == 0 but for the test of v_j(q): where w * w or sumw * sumw leaves
 * float32's range while sum / sumw does not -- a caller's normal near 3e38, a sumw below 2^-75 -- v becomes inf or a NaN and the
 * pixel is no one's tap from then on.)
 * Feedback: after pass feedback_pass - 1, feedback[p].rgb = valid ? i_{feedback_pass}(p)_k * den_k : color[p].rgb, and .w is the
 * bits of color[p].w: the colours SVGF carries into the next frame's history (feedback_pass 1).  It is a range of its own; the
 * caller copies it into plane 0.
 * Finish: out[p].rgb = valid ? i_passes(p)_k * den_k : color[p].rgb; out[p].w = color[p].w, its bits kept; variance_out[p] = valid ?
 * v_passes(p) * (ld * ld) : 0; image[p] (optional, RGBA8) is the tone map of rdx_accumulate on out[p].rgb, with RDX_DENOISE_DEBUG
 * as its debug bit.  passes == 0 is prepare and finish alone.  A pixel's result depends on this order of taps only, not on how the
 * work is cut into launches and blocks.
 * `work` is rdx_svgf_work_size(width, height) bytes of the caller's (the limits of rdx_denoise_work_size; at most 64 bytes per
 * pixel); its contents before and after a call are unspecified.  Nothing is staged and nothing is allocated per call; the call
 * blocks and runs on logical device 0 in multi-device mode.  rdx_get_trace_stats().ms_accumulate is the kernel time of the call.
 * Refused, before anything is launched: an uninitialised library; a NULL or unknown handle among color / moments / materials /
 * surfaces / work / out, an unknown one among variance_out / feedback / image; `settings` NULL, passes > 8, normal_squarings > 7,
 * a sigma_position or sigma_luminance that is negative, infinite or a NaN, an epsilon that is not finite or not > 0, feedback_pass >
 * passes, `feedback` given with feedback_pass == 0 or missing with feedback_pass != 0, unknown flag bits, non-zero padding; a size
 * outside the limits; an offset that is not a multiple of 16 (4 for `image` and `variance_out`); a range that does not hold width x
 * height records (16 per pixel for color / moments / out / feedback, 64 for materials / surfaces, 4 for variance_out / image, the
 * work size); `work`, `out`, `variance_out`, `feedback` or `image` overlapping an input range or each other; wrapped memory that is
 * misaligned.  width == 0 or height == 0 succeeds and touches nothing.
 * Dividing the variance by ld * ld is an approximation: a history holds modulated colours, so its variance is that of albedo times
 * irradiance, and only where the albedo is constant across the frames and taps behind it is variance / ld^2 the variance of l(i).
 * Not covered: a firefly clamp; the exp kernel of the paper (wc is the rational 1 / (1 + x^2), which needs no transcendental);
 * writing the feedback into the history (it is a separate range the caller copies); demodulated histories; guides beyond the
 * primary hit. */
typedef struct rdx_svgf_settings {         /* 32 B */
    uint32_t passes;             /* 0 .. 8: pass j uses step 1 << j */
    uint32_t normal_squarings;   /* 0 .. 7, as rdx_denoise */
    float    sigma_position;     /* as rdx_denoise; 0 = term off */
    float    sigma_luminance;    /* in standard deviations (SVGF: 4); 0 = term off; otherwise finite and > 0 */
    float    epsilon;            /* finite and > 0: added to sigma_luminance * sd */
    uint32_t feedback_pass;      /* 0 = no feedback; otherwise 1 .. passes: `feedback` receives the iterate after that many passes (SVGF: 1) */
    uint32_t flags;              /* RDX_DENOISE_DEMODULATE | RDX_DENOISE_DEBUG, the same bits */
    uint32_t _0;                 /* must be 0 */
} rdx_svgf_settings;
size_t      rdx_svgf_work_size(uint32_t width, uint32_t height);
int         rdx_svgf_filter(rdx_buffer color, size_t color_offset,               /* float4 per pixel, row-major, rgb + w */
                            rdx_buffer moments, size_t moments_offset,           /* float4 per pixel: .z = the luminance variance */
                            rdx_buffer materials, size_t materials_offset,       /* rdx_material_record per pixel */
                            rdx_buffer surfaces, size_t surfaces_offset,         /* rdx_surface per pixel */
                            uint32_t width, uint32_t height, const rdx_svgf_settings* settings,
                            rdx_buffer work, size_t work_offset,                 /* rdx_svgf_work_size bytes; contents before and after unspecified */
                            rdx_buffer out, size_t out_offset,                   /* float4 per pixel */
                            rdx_buffer variance_out, size_t variance_out_offset, /* optional: one float per pixel */
                            rdx_buffer feedback, size_t feedback_offset,         /* optional float4 per pixel; given iff feedback_pass != 0 */
                            rdx_buffer image, size_t image_offset);              /* optional RGBA8 per pixel */
/* Test and measurement seam: bit j of `mask` (j = 0, 1: steps 1 and 2) makes that pass of every later rdx_svgf_filter take its taps
 * from an LDS tile of the block's pixels and their halo, a clear bit straight from memory.  Both forms give the same bits; the
 * default is 3. */
void        rdx_debug_svgf_tiled(uint32_t mask);

/* Test seam: the one rule every call from rdx_query_rays to rdx_trace_paths_env applies to the byte ranges it is given, on plain
 * numbers (needs no device and no initialised library; no address is dereferenced) -> 0, or -1 with the refusal in
 * rdx_last_error().  A row is one range: `bytes` at `offset` of a buffer of `size` bytes at `address`; `align` (a power of two)
 * is the multiple required of the offset and of the address; present == 0: an optional buffer that was not given, the row is
 * skipped.  Rows from first_out on are written: none may overlap a row before it; rows before first_out may overlap each other.
 * Refused, in this order: an offset that is no multiple of its row's align (every row, before any size); offset > size or
 * bytes > size - offset; then, only if n != 0: an address that is no multiple of its row's align; an overlap. */
typedef struct rdx_debug_range { uint64_t address, size, offset, bytes; uint32_t align, present; } rdx_debug_range;
int         rdx_debug_check_ranges(const rdx_debug_range* rows, const char* const* names, uint32_t count, uint32_t first_out,
                                   uint32_t n);

/* Test seams: run single stages on caller-supplied batches (device or host pointers are NOT
 * accepted -- plain host arrays in, host arrays out; the library stages them through HBM). */
typedef struct rdx_hit {
    float    hitPoint[3];
    float    distance;
    uint32_t primitiveIndex, instanceIndex, instanceCustomIndex, instanceSBTOffset;
    float    barycentric[3];
    uint32_t hit;
    float    transform[16];
} rdx_hit;      /* mirrors struct HitData, radiance/shader/radiance.cl:8-18 (+ the hit flag) */
/* mode 0: production kernel (wide nodes, fast slab test; for sbtRecordOffset 2 only `hit` is
 *         meaningful -- any accepted candidate ends a shadow ray);
 * mode 1: reference-order kernel (the reference's own DFS order: full HitData also for shadow rays).
 * visit4 (optional, implies mode 1): {top_nodes, instances, bot_nodes, triangles} visit counts of
 * the reference algorithm summed over the batch. */
int         rdx_trace_batch(rdx_buffer tlas, const float* origins_xyz, const float* dirs_xyz, uint32_t n,
                            float tmin, float tmax, int sbtRecordOffset, int mode, rdx_hit* out, uint64_t* visit4);
typedef struct rdx_payload {
    float color[3]; uint32_t hit; float nextFactor[3]; float nextRayOrigin[3]; float nextRayDirection[3];
} rdx_payload;  /* mirrors struct Payload, samples/shader.cl:4-13 */
/* closest-hit `material` (samples/shader.cl:482-541) on captured hits, using the bound descriptors */
int         rdx_material_batch(const rdx_hit* hits, const float* ray_dirs_xyz, const uint32_t* pixels,
                               const uint32_t* frame_ids, const int32_t* depths, uint32_t n, rdx_payload* out);
/* primary rays (samples/shader.cl:111-173) for explicit pixels / rng inputs, using the bound camera */
int         rdx_generate_batch(const uint32_t* pixels, const uint32_t* rand_in3, uint32_t n,
                               float* origins_xyz, float* dirs_xyz);
int         rdx_pcg3d_batch(const uint32_t* in3, float* out3, uint32_t n);
/* the frame path's per-bounce ray sort on `capacity` device keys of 15 bits (uint16), the first `live` of them alive: perm[0 .. live)
 * = their numbers ordered by the key reduced to key_bits (12, 13 or 14) bits; the order inside a reduced key is unspecified */
int         rdx_debug_sort_keys(rdx_buffer keys, size_t keys_offset, uint32_t live, uint32_t capacity, uint32_t key_bits,
                                rdx_buffer perm, size_t perm_offset);

/* Scalars of the traversal layout derived from a TLAS blob (csrc/accel_layout.h): what the kernels' LDS is sized from and
 * what picks the engine.  Flags are 0 / 1. */
typedef struct rdx_accel_scalars {
    uint32_t stackNeed;                  /* per-lane kernels (reference order: left child followed, right child pushed) */
    uint32_t coopNeed;                   /* wave-cooperative kernel (leaf children are never pushed, smaller subtree first) */
    uint32_t topNeed, blasNeed;          /* its two parts: top-level entries of one ray / entries inside one BLAS (pool engine) */
    uint32_t blasNeedAny;                /* BLAS stack need of the pool engine when the push order depends on the ray (culled walk) */
    uint32_t quadNeed, quadUnifiedNeed;  /* pool-stack need of the quad walk inside one BLAS / from the unified root */
    uint32_t unifiedNeed, unifiedRoot;   /* pool engine: one tree over top level + instances + BLASes, root 0 = not built */
    uint32_t topFlat, topFlatNeed;       /* pool engine: number of top-level nodes if they are few enough (<= 64) to be evaluated
                                          * all at once per ray instead of walked, and the words per lane of the pending-instance bitmap */
    uint32_t nWide;                      /* wide records: inner BLAS nodes of the scene plus the unified tree's (sizes the automatic
                                          * choice of the culled walk) */
    uint32_t nInst;
    uint32_t groupCount;                 /* instances in the shared-transform group */
    uint32_t leafRoots;                  /* flag: some instance's BLAS is a single leaf of <= 8 triangles */
    uint32_t sbtOffsets;                 /* flag: reference-order kernel only (an instance's SBT offset needs the reference's visiting
                                          * order, or a leaf has more triangles than a wide record counts) */
    uint32_t groupIdentity;              /* flag: the group's transform is the identity: root tests in the flat top-level step */
    uint32_t coopOK;                     /* flag: the scene fits the packed words of the cooperative engines (the runtime also
                                          * requires that their LDS footprint fits) */
    float    sceneLo[3], sceneHi[3];     /* box of the top-level root (per-bounce ray sort grid) */
} rdx_accel_scalars;
/* Test seam: derives the layout of `blob` on the host under options "quad" / "cull" (-1, 0, 1 as in rdx_set_option).  Needs no
 * device and no initialised library.  The eight derived arrays are, in this order: top-level nodes, their copy ordered for the
 * cooperative kernel, instances, BLAS nodes, triangles, wide records, quad records, group bitmap (csrc/rdx_types.h layouts).
 * `bytes` (optional, 8 entries) receives their sizes in bytes.  `arrays` (optional, 8 entries, needs `bytes`): every non-null
 * entry receives that array; the caller states its capacity in bytes[i], from a size query made before. */
int         rdx_debug_accel_layout(const void* blob, size_t size, int quad, int cull, rdx_accel_scalars* scalars,
                                   void* const* arrays, size_t* bytes);

/* Test seam: the layout of blobs[count - 1], reached the way rdx_tlas_update reaches it -- blobs[0] derived afresh, then one update
 * per further blob (csrc/accel_layout.h update_accel_layout, owner words and wide tail written on the host).  Output as above.
 * path_per_step (optional, count - 1 entries): 1 = that step was incremental, 2 = it took the full derivation.  Needs no device. */
int         rdx_debug_accel_layout_update(const void* const* blobs, const size_t* sizes, uint32_t count, int quad, int cull,
                                          rdx_accel_scalars* scalars, void* const* arrays, size_t* bytes, uint32_t* path_per_step);


/* Test seam: the entry records of the layout of blobs[count - 1], reached like rdx_debug_accel_layout_update reaches it (count 1: a
 * plain derivation) -- one 128-byte quad record per instance slot (csrc/accel_layout.h AccelLayout::entries; none without quad
 * records), which the runtime keeps behind the quad records on the device -- and, in *need (optional), the pool need of a walk
 * that starts at one.  *bytes: in, the capacity of `entries` (ignored when `entries` is NULL: a size query); out, their size. */
int         rdx_debug_accel_entries(const void* const* blobs, const size_t* sizes, uint32_t count, int quad, int cull,
                                    void* entries, size_t* bytes, uint32_t* need);

#ifdef __cplusplus
}
#endif
#endif /* RDX_H */

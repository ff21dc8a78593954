/* user_paths.cl -- a user program that runs in BOTH modes of the run-time shader compiler: as the megakernel it is
 * (rdx_set_option("user_stages", 0): the `raygen` below, one work-item per pixel, through the product's own device library) and
 * with its stage functions on the wavefront pipeline ("user_stages" 2: `raygen` is then not used; the pipeline's generate /
 * stage / accumulate kernels are the loop).  tests/test_gpu_user_stage_parity.py holds the two frames to each other bit for
 * bit.  Own text, written against the shader interface (radiance.cl / pbr.cl / math.cl of the product's shader directory).
 *
 * The test puts `#define VARIANT n` in front of this text; VARIANT selects the bodies of `material` (row 1) and `environment`
 * (miss 3).  The shadow row (row 2: closest-hit `shadow`, any-hit `anyShadow`) and `shadowMiss` (miss 4) are the same in all.
 *
 * Primary rays are not computed here: descriptor slot 8 (uvData; the pipeline does not read it with option "textures" 0) holds
 * the rays of rdx_generate_rays for every sample of the call, 8 floats per ray (origin | tmin, direction | tmax), sample-major,
 * so both modes start from the same bits.
 *
 * `events` is the program's own bookkeeping, carried in its own Payload: the shaders count their invocations, the megakernel's
 * raygen folds them into channel 3 of imageScratch (the pipeline's accumulate stage leaves that channel alone; stage mode never
 * initialises or reads the field).  The test reads the inputs' coverage from it; only RGB is compared.
 *   bit 0  a closest-hit shader ran              bit 4  a closest-hit shader returned hit = false after depth 0
 *   bit 1  a closest-hit shader queried          bit 5  the miss shader returned hit = true
 *   bit 2  a query was answered "hit"            bit 6  a ray was traced at the last depth
 *   bit 3  a closest-hit shader returned         bit 7  the miss shader ran
 *          hit = false at depth 0
 *   bits 8-11 / 12-15 / 16-19: closest-hit invocations / queries / queries answered "hit" of the pixel (all samples of the call)
 */
#include "radiance.cl"
#include "pbr.cl"
#include "math.cl"

#ifndef VARIANT
#define VARIANT 1
#endif

#define EV_HIT_RAN 1u
#define EV_QUERIED 2u
#define EV_ANSWER_HIT 4u
#define EV_FALSE_AT_0 8u
#define EV_FALSE_LATER 16u
#define EV_MISS_CONTINUED 32u
#define EV_LAST_DEPTH 64u
#define EV_MISS_RAN 128u
#define EV_COUNT_HIT (1u << 8)
#define EV_COUNT_QUERY (1u << 12)
#define EV_COUNT_ANSWER (1u << 16)

struct Payload { float3 color; bool hit; float3 nextFactor; float3 nextRayOrigin; float3 nextRayDirection; uint events; };
struct PhysicalCamera { float widthPixel, heightPixel, focalLength, sensorWidth, focalDistance, fStop, x, y, z, wx, wy, wz; };
struct SceneData {
    __global struct PhysicalCamera* camData; __global struct SceneProperties* scene; __global struct MeshInfo* meshInfoData;
    __global float* vertexData; __global uint* indexData; __global float* uvData; __global float* normalData;
    __global struct Material* materials; __global struct AccelStruct* topLevel;
    int depth; unsigned int frameID; unsigned int debug;
};

#if VARIANT == 11
#define QUERY_MISS 3
#else
#define QUERY_MISS 4
#endif

/* ---- what the variants share ------------------------------------------------------------------------------------------------ */
struct Surface { float3 P, N, L, O, tint, light; };

/* the hit in world space, a stand-in normal that faces the ray, the light, a query origin off the surface, a colour per primitive */
void surfaceOf(struct Surface* s, struct Payload* payload, struct HitData* hitData, struct SceneData* sceneData)
{
    const float16 m = hitData->transform;
    const float3 h = hitData->hitPoint;
    s->P = (float3)(m.s0 * h.x + m.s1 * h.y + m.s2 * h.z + m.s3, m.s4 * h.x + m.s5 * h.y + m.s6 * h.z + m.s7,
                    m.s8 * h.x + m.s9 * h.y + m.sa * h.z + m.sb);
    const float3 back = -normalize(payload->nextRayDirection);
    s->N = normalize(back + 0.3f * (hitData->barycentric.yzx - (float3)(1.0f / 3.0f)));
    s->L = normalize(-sceneData->scene->lights[0].direction.xyz);
    s->O = s->P + 0.02f * s->N;
    s->tint = (float3)(0.25f + (float)(hitData->primitiveIndex % 5u) / 8.0f, 0.25f + (float)(hitData->instanceIndex % 3u) / 4.0f,
                       0.25f + (float)(hitData->instanceCustomIndex % 4u) / 6.0f);
    s->light = sceneData->scene->lights[0].color.xyz;
}

/* a direction that depends on the hit and the depth only: somewhere in the hemisphere around n, and into the scene */
float3 scatterOf(struct Surface* s, struct HitData* hitData, struct SceneData* sceneData)
{
    const float3 r = random_pcg3d((uint3)(hitData->primitiveIndex, hitData->instanceIndex + 17u, (uint)sceneData->depth));
    return normalize(s->N + 1.6f * (r - 0.5f));
}

/* a query payload with every field set: the callbacks of a query may read any of them */
struct Payload queryFor(struct Surface* s)
{
    struct Payload q;
    q.color = (float3)(0.0f); q.hit = false; q.nextFactor = (float3)(1.0f); q.nextRayOrigin = s->O; q.nextRayDirection = s->L; q.events = 0u;
    return q;
}

#define ASK(q) traceRay(sceneData->topLevel, 2, QUERY_MISS, s.O, s.L, 0.001f, 1000, &(q), sceneData, imageArray, sampler)
#define NOTE_QUERY(q) (payload->events = (payload->events | EV_QUERIED | ((q).hit ? EV_ANSWER_HIT : 0u)) + EV_COUNT_QUERY + ((q).hit ? EV_COUNT_ANSWER : 0u))

/* ---- row 1: the closest-hit shader ------------------------------------------------------------------------------------------- */
void material(struct Payload* payload, struct HitData* hitData, struct SceneData* sceneData, image2d_array_t imageArray, sampler_t sampler)
{
#if VARIANT == 3
    /* query_steers: the query comes first; its answer chooses the next ray and the throughput, one of them with a zero */
    struct Surface s;
    surfaceOf(&s, payload, hitData, sceneData);
    struct Payload query = queryFor(&s);
    ASK(query);
    payload->events = (payload->events | EV_HIT_RAN) + EV_COUNT_HIT;
    NOTE_QUERY(query);
    payload->hit = true;
    payload->color = 0.15f * s.tint;
    payload->nextRayOrigin = s.O;
    if (query.hit) {
        payload->nextRayDirection = normalize(s.N + 0.8f * cross(s.N, s.L));
        payload->nextFactor = (float3)(0.9f, 0.0f, 0.6f) * s.tint;
    } else {
        payload->color += s.tint * max(dot(s.N, s.L), 0.0f) * s.light;
        payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
        payload->nextFactor = (float3)(0.5f, 0.7f, 0.9f);
    }
#else
    struct Surface s;
    surfaceOf(&s, payload, hitData, sceneData);
    payload->events = (payload->events | EV_HIT_RAN) + EV_COUNT_HIT;
#if VARIANT == 1
    /* no_query */
    payload->hit = true;
    payload->color = 0.2f * s.tint + 0.5f * s.tint * max(dot(s.N, s.L), 0.0f) * s.light;
    payload->nextRayOrigin = s.O;
    payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
    payload->nextFactor = 0.6f * s.tint + 0.2f;
#elif VARIANT == 2
    /* query_some: only hits on even primitives ask; the others decide by the angle alone and must not see a neighbour's answer */
    bool lit = dot(s.N, s.L) > 0.3f;
    if ((hitData->primitiveIndex & 1u) == 0u) {
        struct Payload query = queryFor(&s);
        ASK(query);
        NOTE_QUERY(query);
        lit = !query.hit;
    }
    payload->hit = true;
    payload->color = 0.1f * s.tint + (lit ? s.tint * (0.25f + max(dot(s.N, s.L), 0.0f)) * s.light : (float3)(0.0f));
    payload->nextRayOrigin = s.O;
    payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
    payload->nextFactor = lit ? 0.7f * s.tint : 0.4f * s.tint + 0.3f;
#elif VARIANT == 4
    /* query_last: everything is written first; the query, on the payload itself, is the last statement: the shadow row answers
     * hit = true, color = 0 or hit = false, color = 1, and the next ray and the factor written before it stay */
    payload->hit = true;
    payload->color = 0.3f * s.tint;
    payload->nextRayOrigin = s.O;
    payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
    payload->nextFactor = 0.5f * s.tint + 0.4f;
    payload->events = (payload->events | EV_QUERIED) + EV_COUNT_QUERY;
    ASK(*payload);
#elif VARIANT == 5
    /* payload_carry: builds on what the previous bounce (at depth 0: the raygen) left in the payload */
    const float3 beforeC = payload->color, beforeF = payload->nextFactor, beforeO = payload->nextRayOrigin, beforeD = payload->nextRayDirection;
    struct Payload query = queryFor(&s);
    ASK(query);
    NOTE_QUERY(query);
    payload->hit = true;
    payload->color = 0.5f * beforeC + 0.1f * s.tint + (query.hit ? (float3)(0.0f) : 0.5f * s.tint * max(dot(s.N, s.L), 0.0f) * s.light);
    payload->nextFactor = 0.5f * beforeF + 0.4f * s.tint;
    payload->nextRayOrigin = s.O + 0.001f * normalize(beforeO - s.P);
    payload->nextRayDirection = normalize(scatterOf(&s, hitData, sceneData) + 0.2f * normalize(beforeD));
#elif VARIANT == 6
    /* hit_false: by primitive, instance and depth, a quarter of the hits say "no hit" -- three quarters at depth 1, so that scenes
     * whose paths seldom live longer see it after depth 0 as well -- and still leave a colour and a next ray */
    struct Payload query = queryFor(&s);
    ASK(query);
    NOTE_QUERY(query);
    const bool quarter = ((hitData->primitiveIndex + hitData->instanceIndex + (uint)sceneData->depth) & 3u) == 0u;
    payload->hit = sceneData->depth == 1 ? quarter : !quarter;
    payload->color = 0.2f * s.tint + (query.hit ? (float3)(0.0f) : 0.6f * s.tint * max(dot(s.N, s.L), 0.0f) * s.light);
    payload->nextRayOrigin = s.O;
    payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
    payload->nextFactor = 0.6f * s.tint + 0.3f;
#elif VARIANT == 8
    /* pixel_rng: the per-pixel random numbers drive the next ray */
    struct Payload query = queryFor(&s);
    ASK(query);
    NOTE_QUERY(query);
    const float3 r = random_pcg3d((uint3)(sceneData->frameID, (uint)get_global_id(0), (uint)sceneData->depth));
    payload->hit = true;
    payload->color = 0.1f * s.tint + (query.hit ? (float3)(0.0f) : r.z * s.tint * max(dot(s.N, s.L), 0.0f) * s.light);
    payload->nextRayOrigin = s.O;
    payload->nextRayDirection = normalize(s.N + 1.8f * (r - 0.5f));
    payload->nextFactor = 0.5f * s.tint + 0.5f * r.yzx;
#elif VARIANT == 9
    /* reads_interface: every SceneData pointer, every HitData field */
    __global struct MeshInfo* mesh = sceneData->meshInfoData + hitData->instanceIndex;
    __global struct Material* mat = sceneData->materials + mesh->materialIndex;
    float3 corner[3], normalAt[3];
    for (int k = 0; k < 3; ++k) {
        const uint v = sceneData->indexData[mesh->indexOffset + 3 * hitData->primitiveIndex + k];
        corner[k] = vload3(0, sceneData->vertexData + mesh->vertexOffset + 3 * v);
        normalAt[k] = vload3(0, sceneData->normalData + mesh->normalOffset + 3 * v);
    }
    const float3 b = hitData->barycentric;
    const float3 objectPoint = b.x * corner[0] + b.y * corner[1] + b.z * corner[2];
    const float3 shadingNormal = b.x * normalAt[0] + b.y * normalAt[1] + b.z * normalAt[2];
    const float16 m = hitData->transform;
    const float3 Nw = normalize((float3)(m.s0 * shadingNormal.x + m.s1 * shadingNormal.y + m.s2 * shadingNormal.z,
                                         m.s4 * shadingNormal.x + m.s5 * shadingNormal.y + m.s6 * shadingNormal.z,
                                         m.s8 * shadingNormal.x + m.s9 * shadingNormal.y + m.sa * shadingNormal.z) + 0.001f * s.N);
    struct Payload query = queryFor(&s);
    ASK(query);
    NOTE_QUERY(query);
    float3 extra = (float3)(0.0f);
    for (uint k = 1u; k < 5u; ++k)
        extra += (k < sceneData->scene->lightCount.x ? 1.0f : 0.125f) * sceneData->scene->lights[k].color.xyz
                 * max(dot(Nw, -sceneData->scene->lights[k].direction.xyz), 0.0f);
    __global struct PhysicalCamera* cam = sceneData->camData;
    const float3 toEye = normalize((float3)(cam->x, cam->y, cam->z) - s.P);
    const uint4 texel = read_imageui(imageArray, sampler, (float4)(b.y, b.z, (float)(hitData->primitiveIndex % 3u), 0.0f));
    const float3 albedo = mat->albedo.xyz * (0.5f + convert_float3(texel.xyz) / 510.0f);
    payload->hit = true;
    payload->color = albedo * (0.1f + 0.05f * mat->roughness + (float)hitData->instanceCustomIndex / 16.0f)
                     + (query.hit ? (float3)(0.0f) : albedo * max(dot(Nw, s.L), 0.0f) * s.light) + extra
                     + 0.05f * max(dot(Nw, toEye), 0.0f) * (cam->focalLength / cam->sensorWidth)
                     + 0.01f * fabs(objectPoint - hitData->hitPoint) + 0.001f * fmin(hitData->distance, 10.0f);
    payload->nextRayOrigin = s.P + 0.02f * Nw * (dot(Nw, s.N) < 0.0f ? -1.0f : 1.0f);
    payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
    payload->nextFactor = 0.7f * albedo + 0.1f * mat->metallic;
#else
    /* variants 7 (miss_continues), 10 (scaled_dirs), 11 (shadow_miss_3): a lit surface with the stock query in the middle */
    struct Payload query = queryFor(&s);
    ASK(query);
    NOTE_QUERY(query);
    payload->hit = true;
    payload->color = 0.1f * s.tint + (query.hit ? (float3)(0.0f) : s.tint * max(dot(s.N, s.L), 0.0f) * s.light * query.color);
    payload->nextRayOrigin = s.O;
    payload->nextRayDirection = scatterOf(&s, hitData, sceneData);
#if VARIANT == 10
    /* left unnormalised: a thousand times too short or too long, by primitive */
    payload->nextRayDirection *= (hitData->primitiveIndex & 1u) ? 1e3f : 1e-3f;
#endif
    payload->nextFactor = 0.6f * s.tint + 0.2f;
#endif
#endif
}

/* ---- miss 3: the environment ------------------------------------------------------------------------------------------------- */
void environment(struct Payload* payload, struct SceneData* sceneData, image2d_array_t imageArray, sampler_t sampler)
{
    const float3 d = normalize(payload->nextRayDirection);
#if VARIANT == 7
    /* miss_continues: colour by direction, depth, frame and pixel; the upper half continues at even depths, the lower at odd ones */
    const uint g = (uint)get_global_id(0);
    payload->color = 0.5f * (float3)(0.5f + 0.5f * d.x, 0.2f * (float)(sceneData->depth + 1), (float)((g + 5u * sceneData->frameID) % 16u) / 16.0f);
    payload->hit = (d.y > 0.0f) != ((sceneData->depth & 1) != 0);
    if (payload->hit) payload->nextFactor = (float3)(0.9f, 0.8f, 0.7f);
#elif VARIANT == 8
    /* pixel_rng: the random numbers decide whether the path goes on, and where to */
    const float3 r = random_pcg3d((uint3)(sceneData->frameID, (uint)get_global_id(0), (uint)sceneData->depth));
    payload->color = (float3)(0.3f, 0.4f, 0.6f) * (0.5f + 0.5f * r.y);
    payload->hit = r.x < 0.5f;
    payload->nextRayDirection = normalize(2.0f * r - 1.0f);
    payload->nextFactor = (float3)(0.8f);
#else
    payload->color = (float3)(0.2f, 0.3f, 0.5f) + 0.5f * max(d.y, 0.0f);
    payload->hit = false;
#endif
}

/* ---- row 2 and miss 4: the shadow query -------------------------------------------------------------------------------------- */
void shadow(struct Payload* payload) { payload->hit = true; payload->color = 0.0f; }
void shadowMiss(struct Payload* payload) { payload->hit = false; payload->color = 1.0f; }

void callHit(int sbtRecordOffset, struct Payload* payload, struct HitData* hitData, struct SceneData* sceneData, image2d_array_t imageArray, sampler_t sampler)
{
    const int row = (int)hitData->instanceSBTOffset + sbtRecordOffset;
    if (row == 1) material(payload, hitData, sceneData, imageArray, sampler);
    else if (row == 2) shadow(payload);
}
void callAnyHit(bool* cont, int sbtRecordOffset, struct Payload* payload, struct HitData* hitData, struct SceneData* sceneData, image2d_array_t imageArray, sampler_t sampler)
{
    if ((int)hitData->instanceSBTOffset + sbtRecordOffset == 2) *cont = false;   /* the first candidate ends a shadow ray */
}
void callMiss(int missIndex, struct Payload* payload, struct SceneData* sceneData, image2d_array_t imageArray, sampler_t sampler)
{
    if (missIndex == 3) environment(payload, sceneData, imageArray, sampler);
    else if (missIndex == 4) shadowMiss(payload);
}

/* ---- the megakernel: one pixel, every sample of the call --------------------------------------------------------------------- */
__kernel void raygen(__global struct RayTraceProperties* RTProp, __global float* imageScratch, __global uchar* image,
                     __global struct PhysicalCamera* camData, __global struct SceneProperties* scene, __global struct MeshInfo* meshInfoData,
                     __global float* vertexData, __global uint* indexData, __global float* uvData, __global float* normalData,
                     __global struct Material* materials, image2d_array_t imageArray, sampler_t sampler, __global struct AccelStruct* topLevel)
{
    const uint pixel = (uint)get_global_id(0);
    const uint nPixels = (uint)camData->widthPixel * (uint)camData->heightPixel;
    const uint firstSample = RTProp->totalSamples, nSamples = RTProp->batchSize, maxDepth = RTProp->depth, debug = RTProp->debug;
    __global float* mean = imageScratch + 4 * (size_t)pixel;
    uint seen = 0u;
    for (uint k = 0u; k < nSamples; ++k) {
        const uint frameID = firstSample + k;
        __global const float* primary = uvData + 8 * ((size_t)k * nPixels + pixel);
        struct SceneData sd;
        sd.camData = camData; sd.scene = scene; sd.meshInfoData = meshInfoData; sd.vertexData = vertexData; sd.indexData = indexData;
        sd.uvData = uvData; sd.normalData = normalData; sd.materials = materials; sd.topLevel = topLevel;
        sd.depth = 0; sd.frameID = frameID; sd.debug = debug;
        struct Payload payload;
        payload.color = (float3)(0.0f); payload.hit = false; payload.nextFactor = (float3)(1.0f);
        payload.nextRayOrigin = (float3)(primary[0], primary[1], primary[2]);
        payload.nextRayDirection = (float3)(primary[4], primary[5], primary[6]);
        payload.events = 0u;
        float3 radiance = (float3)(0.0f), weight = (float3)(1.0f);
        while ((uint)sd.depth < maxDepth) {
            const uint ranBefore = payload.events & (15u << 8);
            if ((uint)sd.depth + 1u == maxDepth) payload.events |= EV_LAST_DEPTH;
            traceRay(topLevel, 1, 3, payload.nextRayOrigin, payload.nextRayDirection, 0.001f, 1000, &payload, &sd, imageArray, sampler);
            const bool byHitShader = (payload.events & (15u << 8)) != ranBefore;
            if (!byHitShader) payload.events |= EV_MISS_RAN | (payload.hit ? EV_MISS_CONTINUED : 0u);
            else if (!payload.hit) payload.events |= sd.depth == 0 ? EV_FALSE_AT_0 : EV_FALSE_LATER;
            if (payload.hit) {
                radiance += weight * payload.color;
                weight *= payload.nextFactor;
            } else if (sd.depth == 0) radiance = payload.color;     /* nothing hit by the primary ray: the background, and on */
            else break;                                             /* a later ray that hit nothing ends the path */
            sd.depth++;
            payload.hit = false;
            if (debug) break;
        }
        if (frameID == 0u) { mean[0] = radiance.x; mean[1] = radiance.y; mean[2] = radiance.z; }
        else {
            mean[0] = (frameID * mean[0] + radiance.x) / (frameID + 1);
            mean[1] = (frameID * mean[1] + radiance.y) / (frameID + 1);
            mean[2] = (frameID * mean[2] + radiance.z) / (frameID + 1);
        }
        seen = ((seen | payload.events) & 0xffu) | (((seen >> 8) + (payload.events >> 8)) << 8);
    }
    ((__global uint*)mean)[3] = seen;
}

// area.hip -- device side of rdx_area_light_hits and rdx_trace_paths_area: the direct term of one record of a caller's area light
// table -- a parallelogram or a triangle of constant radiance (include/rdx.h rdx_area_light), sampled at ONE point per (hit, light)
// -- on material records, and the shade kernel of a bounce that samples every record of a punctual table and then every record of
// an area table at every hit:
//
//   closest-hit query -> k_area_shade -> any-hit query of live x (L + A) shadow rays -> k_lights_fold (light_paths.hip, unchanged)
//
// A translation unit of its own, like its siblings and for the same reason: the code objects of the ten existing device units stay
// the ones they were, bit for bit (profiles/area_kernels.txt).  k_area_shade is k_punctual_shade (punctual.hip) with a second
// light loop; its body is restated here operation for operation, as every sibling restates it (DESIGN 4.16 records why a shared
// template was rejected), and punctual_emit is restated with it, because moving it into a header would touch punctual.hip:
// tests/test_gpu_area.py holds the restatement to rdx_trace_paths_punctual bit for bit.  What an area record emits at a hit is ONE
// function, area_emit, for both kernels, so the per-path call has the bits of the per-hit call; the PBR, frame and RNG functions
// are those of stages.h / device_math.h, called as k_light_hits (material.hip) and k_scatter_hits (scatter.hip) call them.
#include "kernels.h"

#include "area.h"
#include "device_math.h"
#include "light_paths.h"
#include "shade.h"
#include "stages.h"
#include "surface.h"

namespace rdx {

constexpr uint32_t AREA_BLOCK = 256;

// punctual.hip's punctual_emit, restated word for word (that unit keeps its function to itself so that its code object does not
// change): record `lt` seen from `above` -> L, E, tmax; false: dark there.
__device__ __forceinline__ bool punctual_emit(const PunctualLight* __restrict__ lt, const f3& above, f3& L, f3& E, float& tmax)
{
    const uint32_t type = lt->type;
    if (type > LIGHT_SPOT) return false;
    E = mk3(lt->color[0], lt->color[1], lt->color[2]);
    if (type == LIGHT_DIRECTIONAL) {
        L = normalize3(mk3(-lt->direction[0], -lt->direction[1], -lt->direction[2]));
        tmax = 1000.0f;
        return true;
    }
    const f3 v = mk3(lt->position[0] - above.x, lt->position[1] - above.y, lt->position[2] - above.z);
    const float d2 = (v.x * v.x + v.y * v.y) + v.z * v.z;
    if (!(d2 > 0.0f)) return false;
    if (!(d2 < __builtin_inff())) return false;
    const float range = lt->range;
    if (range > 0.0f && !(d2 < range * range)) return false;
    L = normalize3(v);
    const float att = 1.0f / d2;
    E = E * att;
    tmax = sqrtf(d2);
    if (type == LIGHT_SPOT) {
        const f3 S = normalize3(mk3(lt->direction[0], lt->direction[1], lt->direction[2]));
        const float c = -((S.x * L.x + S.y * L.y) + S.z * L.z);
        const float f = cl_clamp(c * lt->coneScale + lt->coneOffset, 0.0f, 1.0f);
        if (!(f > 0.0f)) return false;
        E = E * (f * f);
    }
    return true;
}

// Area record `lt` seen from `above` with the random pair (u, v): the point p = corner + u edgeU + v edgeV of the emitter (the pair
// folded into the triangle for type 1), L = the unit direction towards p, E = radiance x (emitter area x cosine at the emitter) /
// distance^2 -- the one-sample estimator under the pdf 1 / area --, tmax = 0.999 of the distance: the shadow ray stops short of the
// emitter.  false: the record is dark there (unknown type, d2 zero or not finite, back face of a one-sided record, degenerate
// emitter, NaN).  n = cross(edgeU, edgeV) is NOT normalised: |n| is the parallelogram's area, so g = -dot(n, L) is area x cosine and
// no square root is taken.  Every float32 operation is rounded on its own (this unit is compiled with -ffp-contract=off), and p, n,
// d2 and g are plain products and sums, NOT dot3 / cross3, which may fuse: numpy float32 restates them (tests/area_cases.py
// `emitted_area`).  `lt` is the same address in every lane, so its sixteen words arrive through the scalar cache and the branches
// on `type` and `flags` are uniform; u, v and everything from p on are per lane.
__device__ __forceinline__ bool area_emit(const AreaLight* __restrict__ lt, const f3& above, float u, float v, f3& L, f3& E, float& tmax)
{
    const uint32_t type = lt->type;
    if (type > AREA_TRIANGLE) return false;
    if (type == AREA_TRIANGLE && u + v > 1.0f) { u = 1.0f - u; v = 1.0f - v; }
    const f3 eu = mk3(lt->edgeU[0], lt->edgeU[1], lt->edgeU[2]), ev = mk3(lt->edgeV[0], lt->edgeV[1], lt->edgeV[2]);
    const f3 p = mk3((lt->corner[0] + eu.x * u) + ev.x * v, (lt->corner[1] + eu.y * u) + ev.y * v, (lt->corner[2] + eu.z * u) + ev.z * v);
    const f3 n = mk3(eu.y * ev.z - eu.z * ev.y, eu.z * ev.x - eu.x * ev.z, eu.x * ev.y - eu.y * ev.x);
    const f3 w = mk3(p.x - above.x, p.y - above.y, p.z - above.z);
    const float d2 = (w.x * w.x + w.y * w.y) + w.z * w.z;
    if (!(d2 > 0.0f)) return false;
    if (!(d2 < __builtin_inff())) return false;
    L = normalize3(w);
    float g = -((n.x * L.x + n.y * L.y) + n.z * L.z);
    if (type == AREA_TRIANGLE) g = g * 0.5f;
    if (lt->flags & AREA_TWO_SIDED) g = fabsf(g);
    if (!(g > 0.0f)) return false;
    const float s = g / d2;
    E = mk3(lt->radiance[0] * s, lt->radiance[1] * s, lt->radiance[2] * s);
    tmax = sqrtf(d2) * 0.999f;
    return true;
}

// One record per thread, as k_punctual_light_hits (punctual.hip): the direction of ray i = rays[2i + 1], material record i =
// mats[4i .. 4i + 3], key i = keys[i] or randoms i = randoms[i] (exactly one of the two pointers is given); lit[i] = (rgb, 0),
// shadow record i = shadow[2i], shadow[2i + 1].  The random pair of the keys route is pcg3d(frameID, pixel, depth + ((stream + 1)
// << 16)).xy: paths are at most 62 deep, so no such third word is the bare depth rdx_scatter_hits draws from, or another stream's.
// Nothing is gathered, so nothing is fenced; no atomics, no LDS.
__global__ void __launch_bounds__(AREA_BLOCK)
k_area_light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, const AreaLight* __restrict__ light,
                  const uint4* __restrict__ keys, uint32_t stream, const float4* __restrict__ randoms, float4* __restrict__ lit,
                  float4* __restrict__ shadow)
{
    const uint32_t i = blockIdx.x * AREA_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 rd = rays[2 * (size_t)i + 1];
    const float4 m0 = mats[4 * (size_t)i], m1 = mats[4 * (size_t)i + 1], m2 = mats[4 * (size_t)i + 2], m3 = mats[4 * (size_t)i + 3];
    // a dark record, any other value of `hit`: zeros (a shadow ray with tmax 0 accepts nothing)
    float4 c = make_float4(0.f, 0.f, 0.f, 0.f), s0 = c, s1 = c;
    if (__float_as_uint(m0.w) == 1u) {
        float u, v;
        if (keys) {
            const uint4 key = keys[i];
            const f3 rnd = pcg3d(key.x, key.y, key.z + ((stream + 1u) << 16));
            u = rnd.x; v = rnd.y;
        } else {
            const float4 r = randoms[i];
            u = r.x; v = r.y;
        }
        const f3 above = mk3(m3.x, m3.y, m3.z);
        f3 L, E;
        float tmax;
        if (area_emit(light, above, u, v, L, E, tmax)) {
            const f3 N = mk3(m0.x, m0.y, m0.z), albedo = mk3(m1.x, m1.y, m1.z);
            const float metallic = m2.x, roughness = m2.y, transmission = m2.z;
            const f3 V = normalize3(-mk3(rd.x, rd.y, rd.z));
            NFrame FN;
            make_frame(N, FN);
            const f3 direct = mk3(0.0f, 0.0f, 0.0f) + microfacet_brdf(FN, L, V, N, albedo, metallic, roughness, transmission) * E;
            c = make_float4(direct.x, direct.y, direct.z, 0.0f);
            s0 = make_float4(above.x, above.y, above.z, 0.001f);
            s1 = make_float4(L.x, L.y, L.z, tmax);
        }
    }
    lit[i] = c;
    if (shadow) { shadow[2 * (size_t)i] = s0; shadow[2 * (size_t)i + 1] = s1; }
}

// k_punctual_shade (punctual.hip) over two tables.  One live ray per lane.  Every gather of a hit is fenced by shade_in_bounds
// (shade.h), asked before and after the index gather exactly as k_resolve_materials asks it, plus the slotOf check; a hit that
// fails is a miss and is counted -- one ballot per wave, one atomic by its first lane, and only where the wave has such a hit.  The
// survivors are compacted by k_scatter_hits' rule -- the survivors of 64 consecutive live rays stay together and in order: a lane's
// record is the block's base from ONE atomic on *live per BLOCK, plus the survivors of the block's earlier waves, plus the lane's
// rank in its wave's ballot.  `lights` and `area` are the tables: the same address in every lane and loop counters that are
// uniform, so each record's sixteen words arrive through the scalar cache; both loops stay rolled.  The tables are the one thing
// the caller's records can point the kernel at, and the host has checked their nLights / nArea records into their buffers.  20
// bytes of LDS: the block's four survivor counts and its base.
__global__ void __launch_bounds__(AREA_BLOCK)
k_area_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc,
             const PunctualLight* __restrict__ lights, uint32_t nLights, const AreaLight* __restrict__ area, uint32_t nArea, LightPathStreams io,
             uint32_t n, uint32_t depth, uint32_t sampleNext, uint32_t* __restrict__ live, uint32_t* __restrict__ invalid)
{
    const uint32_t i = blockIdx.x * AREA_BLOCK + threadIdx.x;
    bool alive = false, bad = false;
    uint4 id = make_uint4(0u, 0u, 0u, 0u);
    float4 w = make_float4(1.0f, 1.0f, 1.0f, 0.0f);
    float4 ro = make_float4(0.f, 0.f, 0.f, 0.f), rd = ro, ha = ro;
    uint32_t prim = 0u, inst = 0u, slot = 0xffffffffu, idx[3] = {0u, 0u, 0u};
    const bool texOn = (sc.tex.flags & TEX_ENABLED) != 0u;
    if (i < n) {
        ro = io.rays[2 * (size_t)i]; rd = io.rays[2 * (size_t)i + 1];
        ha = io.hits[2 * (size_t)i];
        const float4 hb = io.hits[2 * (size_t)i + 1];
        if (depth == 0u) {
            const uint4 key = io.keys[i];
            id = make_uint4(i, key.x, key.y, 0u);
        } else {
            id = io.ids[i];
            w = io.weight[i];
        }
        if (__float_as_uint(ha.w) == 1u) {
            prim = __float_as_uint(hb.x); inst = __float_as_uint(hb.y);
            bool ok = shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, nullptr, sc.s.nIndex, sc.s.nNormal, sc.s.nUv, sc.materials,
                                      sc.nMaterials, texOn, sc.tex.layers);
            if (ok) {
                slot = slotOf[inst];        // 0xffffffff: no instance of the TLAS carries this index (a foreign blob)
                const int64_t first = (int64_t)sc.s.meshInfo[inst].indexOffset + (int64_t)prim * 3;
                idx[0] = sc.s.index[first]; idx[1] = sc.s.index[first + 1]; idx[2] = sc.s.index[first + 2];
                ok = slot < nInst && shade_in_bounds(sc.s.meshInfo, nInst, sc.s.nMeshInfo, inst, prim, idx, sc.s.nIndex, sc.s.nNormal, sc.s.nUv,
                                                     sc.materials, sc.nMaterials, texOn, sc.tex.layers);
            }
            alive = ok;
            bad = !ok;
        }
        // a path's colour starts at zero; a miss at depth 0 shows the stock miss colour (stages.h `environment`)
        if (depth == 0u) io.radiance[i] = alive ? make_float4(0.0f, 0.0f, 0.0f, 0.0f) : make_float4(0.2f, 0.2f, 0.5f, 0.0f);
    }
    // wave64 ballots: every lane of the wave is here (no thread has returned)
    const unsigned long long mb = __ballot(bad);
    if (mb != 0ull && (threadIdx.x & 63u) == 0u) atomicAdd(invalid, (uint32_t)__popcll(mb));
    const unsigned long long m = __ballot(alive);
    const uint32_t lane = __lane_id(), wave = threadIdx.x >> 6;
    // the block's four ballots are summed in LDS and the cursor moves ONCE per block, as in k_lights_shade
    __shared__ uint32_t s_count[AREA_BLOCK / 64], s_base;
    if (lane == 0u) s_count[wave] = (uint32_t)__popcll(m);
    __syncthreads();
    if (threadIdx.x == 0u) {
        uint32_t total = 0u;
        for (uint32_t v = 0; v < AREA_BLOCK / 64; ++v) total += s_count[v];
        s_base = total ? atomicAdd(live, total) : 0u;
    }
    __syncthreads();
    if (!alive) return;
    uint32_t base = s_base;
    for (uint32_t v = 0; v < wave; ++v) base += s_count[v];
    const size_t k = base + (uint32_t)__popcll(m & ((1ull << lane) - 1ull));

    // ---- the material record of k_resolve_materials and the `below` of k_resolve_hits, in registers ----
    const MeshInfo mi = sc.s.meshInfo[inst];
    const Material mt = sc.materials[mi.materialIndex];
    const DInst& I = insts[slot];
    // HitData.hitPoint = localOrigin + localDir * t and barycentric, as kernels.hip fill_hit_info (radiance.cl:243)
    HitInfo h;
    const f3 lo = mat4_mul3(I.inv, ro.x, ro.y, ro.z, 1.0f);
    const f3 ld = mat4_mul3(I.inv, rd.x, rd.y, rd.z, 0.0f);
    h.hitPoint = lo + ld * ha.x;
    h.bx = 1 - ha.y - ha.z; h.by = ha.y; h.bz = ha.z;
    h.primitiveIndex = prim;
    h.instanceIndex = inst;
    h.fwd = I.fwd;
    // interpolated vertex normal -> world by the object->world matrix, w = 0 (shader.cl:340-368); the positions are those
    // shade_in_bounds proved inside, in 64 bits
    const float* nb = sc.s.normal + (int64_t)mi.normalOffset;
    const int64_t v0 = (int64_t)idx[0] * 3, v1 = (int64_t)idx[1] * 3, v2 = (int64_t)idx[2] * 3;
    const f3 n0 = mk3(nb[v0], nb[v0 + 1], nb[v0 + 2]);
    const f3 n1 = mk3(nb[v1], nb[v1 + 1], nb[v1 + 2]);
    const f3 n2 = mk3(nb[v2], nb[v2 + 1], nb[v2 + 2]);
    const f3 nl = mk3(h.bx * n0.x + h.by * n1.x + h.bz * n2.x, h.bx * n0.y + h.by * n1.y + h.bz * n2.y,
                      h.bx * n0.z + h.by * n1.z + h.bz * n2.z);
    const float nw = h.bx * 0.0f + h.by * 0.0f + h.bz * 0.0f;
    const f3 faceN = normalize3(mat4_mul3(h.fwd, nl.x, nl.y, nl.z, nw));
    // getHitPosition(hitData, +-faceN) (shader.cl:453-468): transform * (hitPoint, 1), pushed off the surface along N and along -N
    const f3 P = mat4_mul3(h.fwd, h.hitPoint.x, h.hitPoint.y, h.hitPoint.z, 1.0f);
    const f3 above = P + faceN * 0.00001f;
    const f3 below = P + (-faceN) * 0.00001f;

    // texels are read only when option "textures" is on and an image array is given (TEX_ENABLED); otherwise a material with a
    // texture index sees texel 0, as in the live reference shader (stages.h:255-257)
    float tu = 0.0f, tv = 0.0f;
    if (texOn) {     // getUV, shader.cl:323-338
        const float* ub = sc.s.uv + (int64_t)mi.uvOffset;
        tu = h.bx * ub[v0] + h.by * ub[v1] + h.bz * ub[v2];
        tv = h.bx * ub[v0 + 1] + h.by * ub[v1 + 1] + h.bz * ub[v2 + 1];
    }
    f3 N = faceN;       // getMatNormal, shader.cl:369-395
    if (mt.normalTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.normalTexIdx, tx);
        f4 t; t.x = cl_clamp((float)tx[0] / 255.0f, 0.0f, 1.0f) * 2.0f - 1.0f; t.y = cl_clamp((float)tx[1] / 255.0f, 0.0f, 1.0f) * 2.0f - 1.0f;
        t.z = cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f) * 2.0f - 1.0f; t.w = 0.0f * 2.0f - 1.0f;
        t = normalize4(t);
        float tbn[16];
        normal_space(faceN, tbn);
        N = normalize3(mat4_mul3(tbn, t.x, t.y, t.z, t.w));
    }
    float metallic = mt.metallic;       // getMaterialProp, shader.cl:398-430
    if (mt.metallicTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.metallicTexIdx, tx);
        metallic = cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f);                   // .z (shader.cl:412)
    }
    float roughness = cl_clamp(mt.roughness, 0.0f, 1.0f);
    if (mt.roughnessTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.roughnessTexIdx, tx);
        roughness = cl_clamp((float)tx[1] / 255.0f, 0.05f, 1.0f);                 // .y (shader.cl:422)
    }
    const float transmission = cl_clamp(mt.transmission, 0.0f, 1.0f);
    const float ior = cl_clamp(mt.ior, 0.0f, 10.0f);
    f3 albedo = mk3(mt.albedo[0], mt.albedo[1], mt.albedo[2]);       // getAlbedo, shader.cl:432-451
    if (mt.albedoTexIdx != -1) {
        uint32_t tx[4] = {0u, 0u, 0u, 0u};
        if (texOn) tex_read_ui(sc.tex, tu, 1.0f - tv, (float)mt.albedoTexIdx, tx);
        albedo = mk3(cl_clamp((float)tx[0] / 255.0f, 0.0f, 1.0f), cl_clamp((float)tx[1] / 255.0f, 0.0f, 1.0f), cl_clamp((float)tx[2] / 255.0f, 0.0f, 1.0f));
    }

    // ---- one frame for all lights and the sample (the per-hit kernels and k_scatter_hits each build this one from the record's N) ----
    const f3 V = normalize3(-mk3(rd.x, rd.y, rd.z));
    NFrame FN;
    make_frame(N, FN);

    // ---- records k * (L + A) + j, ray-major: k_punctual_light_hits for record j = 0 .. L - 1, then k_area_light_hits for area
    // record j = 0 .. A - 1 on the keys route with stream = j and the path's own (frame, pixel, depth) ----
    const uint32_t nAll = nLights + nArea;
#pragma unroll 1
    for (uint32_t j = 0; j < nLights; ++j) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), s0 = c, s1 = c;      // a dark record: zeros
        f3 L, E;
        float tmax;
        if (punctual_emit(lights + j, above, L, E, tmax)) {
            const f3 direct = mk3(0.0f, 0.0f, 0.0f) + microfacet_brdf(FN, L, V, N, albedo, metallic, roughness, transmission) * E;
            c = make_float4(direct.x, direct.y, direct.z, 0.0f);
            s0 = make_float4(above.x, above.y, above.z, 0.001f);
            s1 = make_float4(L.x, L.y, L.z, tmax);
        }
        const size_t r = k * nAll + j;
        io.lit[r] = c;
        io.shadow[2 * r] = s0;
        io.shadow[2 * r + 1] = s1;
    }
#pragma unroll 1
    for (uint32_t j = 0; j < nArea; ++j) {
        float4 c = make_float4(0.f, 0.f, 0.f, 0.f), s0 = c, s1 = c;
        const f3 rnd = pcg3d(id.y, id.z, depth + ((j + 1u) << 16));
        f3 L, E;
        float tmax;
        if (area_emit(area + j, above, rnd.x, rnd.y, L, E, tmax)) {
            const f3 direct = mk3(0.0f, 0.0f, 0.0f) + microfacet_brdf(FN, L, V, N, albedo, metallic, roughness, transmission) * E;
            c = make_float4(direct.x, direct.y, direct.z, 0.0f);
            s0 = make_float4(above.x, above.y, above.z, 0.001f);
            s1 = make_float4(L.x, L.y, L.z, tmax);
        }
        const size_t r = k * nAll + nLights + j;
        io.lit[r] = c;
        io.shadow[2 * r] = s0;
        io.shadow[2 * r + 1] = s1;
    }

    // ---- k_scatter_hits with the key (frameID, pixel, depth) ----
    f3 nf = mk3(0.f, 0.f, 0.f);
    if (sampleNext) {
        const f3 rnd = pcg3d(id.y, id.z, depth);
        const f3 nd = sample_brdf_transm(FN, V, N, albedo, metallic, roughness, transmission, ior, rnd, nf);
        const f3 origin = dot3(nd, N) < 0 ? below : above;      // getHitPosition(hitData, -+faceN)
        io.nRays[2 * k] = make_float4(origin.x, origin.y, origin.z, 0.001f);
        io.nRays[2 * k + 1] = make_float4(nd.x, nd.y, nd.z, 1000.0f);
    }
    const f3 ambient = albedo * 0.1f;
    io.nIds[k] = id;
    io.nWeight[k] = w;
    io.foldF[k] = make_float4(nf.x, nf.y, nf.z, 0.0f);
    io.foldA[k] = make_float4(ambient.x, ambient.y, ambient.z, 0.0f);
}

void launch_area_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const AreaLight* light, const uint4* keys,
                            uint32_t stream, const float4* randoms, float4* lit, float4* shadow)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + AREA_BLOCK - 1) / AREA_BLOCK);
    hipLaunchKernelGGL(k_area_light_hits, dim3(blocks), dim3(AREA_BLOCK), 0, st, rays, materials, n, light, keys, stream, randoms, lit, shadow);
}

void launch_area_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                       uint32_t nLights, const AreaLight* area, uint32_t nArea, const LightPathStreams& io, uint32_t n, uint32_t depth, bool sampleNext,
                       uint32_t* live, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + AREA_BLOCK - 1) / AREA_BLOCK);
    hipLaunchKernelGGL(k_area_shade, dim3(blocks), dim3(AREA_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, area, nArea, io, n, depth,
                       sampleNext ? 1u : 0u, live, invalid);
}

} // namespace rdx

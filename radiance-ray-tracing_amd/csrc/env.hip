// env.hip -- device side of the environment calls (include/rdx.h): the sampling table of a lat-long image, built by
// three stream-ordered launches with no host round trip between them --
//
//   k_env_max   grid-stride maximum of the texel weights -> header.wmax     float4 loads, wave reduction, one atomic per block
//   k_env_rows  one block per row: q = the quantised weight, C[y][..] = its inclusive scan, M[y] = the row sum
//   k_env_scan  one block: M = the inclusive scan of the H row sums, header.total = M[H - 1]
//
// -- and the three callers of shared text: k_env_light_hits is light_hits (light_emit.h) around env_emit, k_env_lookup is
// env_lookup per ray, k_env_shade is path_shade.h's body over the punctual table, the area table and the environment, so the
// per-path call has the bits of the per-hit calls.  Maximum and integer sums do not depend on the order they are taken in: the
// table's bytes are a function of the image alone, whatever the grid.  A translation unit of its own, so that the code objects of
// the other units stay the ones they were (profiles/env_kernels.txt).
#include "kernels.h"

#include "env.h"
#include "path_shade.h"

namespace rdx {

constexpr uint32_t ENV_BLOCK = 256;
constexpr uint32_t ENV_WAVES = ENV_BLOCK / 64;

// the larger of two, a NaN if either is one: a texel with a NaN in it has no weight
__device__ __forceinline__ float env_max_nan(float a, float b) { return a > b ? a : (a != a ? a : b); }

// w = max(r, g, b) x the height of the row's band of cos(theta), one product; 0 where that is not finite or not positive
__device__ __forceinline__ float env_weight(const float4& t, const float* __restrict__ rowCos, uint32_t y)
{
    const float w = env_max_nan(t.x, env_max_nan(t.y, t.z)) * (rowCos[y] - rowCos[y + 1u]);
    return (w > 0.0f && w < __builtin_inff()) ? w : 0.0f;
}

// every weight is a non-negative float, whose order is that of its bits: one atomic max per block on the bits, none for a block of
// zeros.  header.wmax is 0 before the launch.
__global__ void __launch_bounds__(ENV_BLOCK)
k_env_max(const float4* __restrict__ image, char* __restrict__ table, uint32_t W, uint32_t H)
{
    const float* __restrict__ rowCos = reinterpret_cast<const float*>(table + env_rowcos_offset());
    const uint32_t texels = W * H, stride = gridDim.x * ENV_BLOCK;
    float m = 0.0f;
    for (uint32_t i = blockIdx.x * ENV_BLOCK + threadIdx.x; i < texels; i += stride) m = fmaxf(m, env_weight(image[i], rowCos, i / W));
    for (int off = 32; off > 0; off >>= 1) m = fmaxf(m, __shfl_xor(m, off));
    __shared__ float s_max[ENV_WAVES];
    if ((threadIdx.x & 63u) == 0u) s_max[threadIdx.x >> 6] = m;
    __syncthreads();
    if (threadIdx.x == 0u) {
        for (uint32_t v = 1; v < ENV_WAVES; ++v) m = fmaxf(m, s_max[v]);
        if (m > 0.0f) atomicMax(reinterpret_cast<uint32_t*>(&reinterpret_cast<EnvHeader*>(table)->wmax), __float_as_uint(m));
    }
}

// Row y = blockIdx.x, in passes of ENV_BLOCK texels: the wave scans its 64 values by cross-lane moves, the four wave totals go
// through LDS, the running sum of the earlier passes is carried in a register.  A row sums to less than 2^30.
__global__ void __launch_bounds__(ENV_BLOCK)
k_env_rows(const float4* __restrict__ image, char* __restrict__ table, uint32_t W, uint32_t H)
{
    const uint32_t y = blockIdx.x;
    const float* __restrict__ rowCos = reinterpret_cast<const float*>(table + env_rowcos_offset());
    uint32_t* __restrict__ Cy = reinterpret_cast<uint32_t*>(table + env_c_offset(H)) + (size_t)y * W;
    const float4* __restrict__ row = image + (size_t)y * W;
    const float scale = 65535.0f / reinterpret_cast<const EnvHeader*>(table)->wmax;       // not used where every weight is 0
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    __shared__ uint32_t s_total[ENV_WAVES];
    uint32_t carry = 0u;
    for (uint32_t base = 0; base < W; base += ENV_BLOCK) {
        const uint32_t x = base + threadIdx.x;
        uint32_t q = 0u;
        if (x < W) {
            const float w = env_weight(row[x], rowCos, y);
            if (w != 0.0f) q = max(1u, min(ENV_QMAX, (uint32_t)(w * scale)));
        }
        uint32_t s = q;
        for (uint32_t off = 1; off < 64u; off <<= 1) {
            const uint32_t below = __shfl_up(s, off);
            if (lane >= off) s += below;
        }
        if (lane == 63u) s_total[wave] = s;
        __syncthreads();
        uint32_t before = 0u, all = 0u;
        for (uint32_t v = 0; v < ENV_WAVES; ++v) {
            const uint32_t t = s_total[v];
            if (v < wave) before += t;
            all += t;
        }
        if (x < W) Cy[x] = carry + before + s;
        carry += all;
        __syncthreads();        // s_total is written again by the next pass
    }
    if (threadIdx.x == 0u) reinterpret_cast<uint64_t*>(table + env_m_offset(W, H))[y] = carry;
}

// One block: thread t owns the ceil(H / ENV_BLOCK) <= 32 consecutive rows from t x that on, sums them, the block scans the 256 sums
// as k_env_rows scans a pass, and the thread writes its rows' inclusive sums over the row sums.
__global__ void __launch_bounds__(ENV_BLOCK)
k_env_scan(char* __restrict__ table, uint32_t W, uint32_t H)
{
    uint64_t* __restrict__ M = reinterpret_cast<uint64_t*>(table + env_m_offset(W, H));
    const uint32_t per = (H + ENV_BLOCK - 1u) / ENV_BLOCK;
    const uint32_t first = min(threadIdx.x * per, H), last = min(first + per, H);
    uint64_t mine = 0ull;
    for (uint32_t y = first; y < last; ++y) mine += M[y];
    const uint32_t lane = threadIdx.x & 63u, wave = threadIdx.x >> 6;
    unsigned long long s = mine;
    for (uint32_t off = 1; off < 64u; off <<= 1) {
        const unsigned long long below = __shfl_up(s, off);
        if (lane >= off) s += below;
    }
    __shared__ unsigned long long s_total[ENV_WAVES];
    if (lane == 63u) s_total[wave] = s;
    __syncthreads();
    uint64_t run = s - mine;       // the rows before this thread's
    for (uint32_t v = 0; v < wave; ++v) run += s_total[v];
    for (uint32_t y = first; y < last; ++y) {
        run += M[y];
        M[y] = run;
    }
    if (last == H && first < H) reinterpret_cast<EnvHeader*>(table)->total = run;
}

// light_hits (light_emit.h) with the environment and key i = keys[i] or randoms i = randoms[i] (exactly one of the two pointers is
// given).  The random triple of the keys route is area_random(frameID, pixel, depth, stream).
__global__ void __launch_bounds__(LIGHT_HITS_BLOCK)
k_env_light_hits(const float4* __restrict__ rays, const float4* __restrict__ mats, uint32_t n, EnvView env, const uint4* __restrict__ keys,
                 uint32_t stream, const float4* __restrict__ randoms, float4* __restrict__ lit, float4* __restrict__ shadow)
{
    light_hits(rays, mats, n, lit, shadow, [=](uint32_t i, const f3&, f3& L, f3& E, float& tmax) {
        f3 rnd;
        if (keys) {
            const uint4 key = keys[i];
            rnd = area_random(key.x, key.y, key.z, stream);
        } else {
            const float4 r = randoms[i];
            rnd = mk3(r.x, r.y, r.z);
        }
        return env_emit(env, rnd.x, rnd.y, rnd.z, L, E, tmax);
    });
}

__global__ void __launch_bounds__(LIGHT_HITS_BLOCK)
k_env_lookup(const float4* __restrict__ rays, uint32_t n, EnvView env, float4* __restrict__ radiance)
{
    const uint32_t i = blockIdx.x * LIGHT_HITS_BLOCK + threadIdx.x;
    if (i >= n) return;
    const float4 rd = rays[2 * (size_t)i + 1];
    radiance[i] = env_lookup(env, mk3(rd.x, rd.y, rd.z));
}

// path_shade over the nLights punctual records, the nArea area records and then the environment: nLights + nArea + 1 records per
// survivor.
__global__ void __launch_bounds__(PATH_SHADE_BLOCK)
k_env_shade(const DInst* __restrict__ insts, const uint32_t* __restrict__ slotOf, uint32_t nInst, ShadeScene sc,
            const PunctualLight* __restrict__ lights, uint32_t nLights, const AreaLight* __restrict__ area, uint32_t nArea, EnvView env,
            LightPathStreams io, uint32_t n, uint32_t depth, uint32_t sampleNext, uint32_t* __restrict__ live, uint32_t* __restrict__ invalid)
{
    path_shade(insts, slotOf, nInst, sc, PunctualAreaEnvSource{lights, nLights, area, nArea, env}, io, n, depth, sampleNext, live, invalid);
}

void launch_env_build(hipStream_t st, const float4* image, char* table, uint32_t w, uint32_t h)
{
    // enough blocks to fill the device for a large image, one per ENV_BLOCK texels for a small one
    const uint32_t blocks = (uint32_t)std::min<uint64_t>(((uint64_t)w * h + ENV_BLOCK - 1) / ENV_BLOCK, 2048);
    hipLaunchKernelGGL(k_env_max, dim3(blocks), dim3(ENV_BLOCK), 0, st, image, table, w, h);
    hipLaunchKernelGGL(k_env_rows, dim3(h), dim3(ENV_BLOCK), 0, st, image, table, w, h);
    hipLaunchKernelGGL(k_env_scan, dim3(1), dim3(ENV_BLOCK), 0, st, table, w, h);
}

void launch_env_light_hits(hipStream_t st, const float4* rays, const float4* materials, uint32_t n, const EnvView& env, const uint4* keys,
                           uint32_t stream, const float4* randoms, float4* lit, float4* shadow)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LIGHT_HITS_BLOCK - 1) / LIGHT_HITS_BLOCK);
    hipLaunchKernelGGL(k_env_light_hits, dim3(blocks), dim3(LIGHT_HITS_BLOCK), 0, st, rays, materials, n, env, keys, stream, randoms, lit, shadow);
}

void launch_env_lookup(hipStream_t st, const float4* rays, uint32_t n, const EnvView& env, float4* radiance)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + LIGHT_HITS_BLOCK - 1) / LIGHT_HITS_BLOCK);
    hipLaunchKernelGGL(k_env_lookup, dim3(blocks), dim3(LIGHT_HITS_BLOCK), 0, st, rays, n, env, radiance);
}

void launch_env_shade(hipStream_t st, const DInst* insts, const uint32_t* slotOf, uint32_t nInst, const ShadeScene& sc, const PunctualLight* lights,
                      uint32_t nLights, const AreaLight* area, uint32_t nArea, const EnvView& env, const LightPathStreams& io, uint32_t n, uint32_t depth,
                      bool sampleNext, uint32_t* live, uint32_t* invalid)
{
    if (!n) return;
    const uint32_t blocks = (uint32_t)(((uint64_t)n + PATH_SHADE_BLOCK - 1) / PATH_SHADE_BLOCK);
    hipLaunchKernelGGL(k_env_shade, dim3(blocks), dim3(PATH_SHADE_BLOCK), 0, st, insts, slotOf, nInst, sc, lights, nLights, area, nArea, env, io, n, depth,
                       sampleNext ? 1u : 0u, live, invalid);
}

} // namespace rdx

// tlas_update.hip -- device side of rdx_tlas_update: the owner words of the triangle records (accel_layout.h AccelOwnerRange).
//
// A translation unit of its own, so that the code object of kernels.hip stays the one it was, bit for bit: a kernel added there
// moves the functions behind it and with them the pc-relative displacements inside the whole-path kernels
// (profiles/tlas_update_kernels.txt).
#include "kernels.h"

#include <algorithm>

namespace rdx {

constexpr uint32_t OWNER_FILL_BLOCK = 256;

// table[r] = {first slot, count, owner, number of slots in the ranges before r}; `total` = slots of all ranges.  Thread i of the
// grid-stride loop finds its range by bisection over the fourth column (a few hundred entries: they stay in cache) and writes
// tris[first + (i - before)]._p0 -- one dword at a 48-byte stride, so a wave's store touches 24 cache lines of 128 bytes whatever
// the mapping: the kernel is bound by those partial-line writes, not by the search.  Slots >= nTris are not written (the host
// checks the table against the array's size; this is the second fence).
__global__ void __launch_bounds__(OWNER_FILL_BLOCK)
k_tri_owner_fill(DTri* __restrict__ tris, uint32_t nTris, const uint4* __restrict__ table, uint32_t nRanges, uint32_t total)
{
    for (uint32_t i = blockIdx.x * OWNER_FILL_BLOCK + threadIdx.x; i < total; i += gridDim.x * OWNER_FILL_BLOCK) {
        uint32_t lo = 0, hi = nRanges;          // the last r with table[r].w <= i
        while (hi - lo > 1u) {
            const uint32_t mid = (lo + hi) >> 1;
            if (table[mid].w <= i) lo = mid; else hi = mid;
        }
        const uint4 r = table[lo];
        const uint32_t k = i - r.w;
        if (k >= r.y) continue;
        const uint32_t slot = r.x + k;
        if (slot < nTris) tris[slot]._p0 = r.z;
    }
}

void launch_tri_owner_fill(hipStream_t st, DTri* tris, uint32_t nTris, const uint4* table, uint32_t nRanges, uint32_t total)
{
    if (!nRanges || !total) return;
    const uint32_t blocks = std::min((total + OWNER_FILL_BLOCK - 1) / OWNER_FILL_BLOCK, 256u * 32u);
    hipLaunchKernelGGL(k_tri_owner_fill, dim3(blocks), dim3(OWNER_FILL_BLOCK), 0, st, tris, nTris, table, nRanges, total);
}

} // namespace rdx

// nr.hip.h — x264 --nr on the device ([x264-upstream] common/quant.c denoise_dct): what the macroblock loop's denoising instantiations (k_mb_slice's NR,
// mb_slice_nr_*.hip) and the primitive x264gpu_denoise_blocks (nr_kernels.hip) share.  A coefficient d at raster index i of a block of category cat
// (0 luma 4x4, 1 luma 8x8, 2 chroma 4x4) becomes  a = |d| - off[cat][i];  d = a < 0 ? 0 : sign(d) * a;  the statistics take |d| as it was.
#pragma once
#include "dsp.hip.h"
#include "dsp8.hip.h"

namespace x264gpu {

// the stream's offsets as the loop stages them: only the 96 entries in use, 192 B — luma 4x4, chroma 4x4, luma 8x8 (16-byte aligned)
constexpr int NR_OFF_N = 96, NR_O4 = 0, NR_OC = 16, NR_O8 = 32;
// dword d < 48 of the staged row <- dword of x264gpu_nr_offsets (off[3][64] uint16)
__device__ __forceinline__ int nr_stage_src(int d) { return d < 8 ? d : d < 16 ? 64 + d - 8 : 32 + d - 16; }

__device__ __forceinline__ int nr_one(int d, int off) { const int a = abs(d) - off; return a < 0 ? 0 : d < 0 ? -a : a; }

// (every function here takes the lane index afresh — relane — so that the addresses it forms are computed where they are used: formed from the macroblock's lane
//  index they are loop invariants of the candidate loop, which the compiler hoists to the macroblock's start and keeps alive across the whole analysis)
// natural layout of a 4x4 block: quad lane & 3 = row, register = column.  off16: the category's offsets (8-byte aligned)
__device__ __forceinline__ void nr_denoise4(int v[4], const uint16_t *off16, int lane)
{
    const int j = relane(lane) & 3;
    const uint2 o = *(const uint2 *)(off16 + j * 4);
    v[0] = nr_one(v[0], (int)(o.x & 0xffffu)); v[1] = nr_one(v[1], (int)(o.x >> 16));
    v[2] = nr_one(v[2], (int)(o.y & 0xffffu)); v[3] = nr_one(v[3], (int)(o.y >> 16));
}
// ... of an 8x8 block: lane & 7 = row, register = column.  off64: category 1's offsets (16-byte aligned)
__device__ __forceinline__ void nr_denoise8(int v[8], const uint16_t *off64, int lane)
{
    const int row = relane(lane) & 7;
    const uint4 o = *(const uint4 *)(off64 + row * 8);
    v[0] = nr_one(v[0], (int)(o.x & 0xffffu)); v[1] = nr_one(v[1], (int)(o.x >> 16));
    v[2] = nr_one(v[2], (int)(o.y & 0xffffu)); v[3] = nr_one(v[3], (int)(o.y >> 16));
    v[4] = nr_one(v[4], (int)(o.z & 0xffffu)); v[5] = nr_one(v[5], (int)(o.z >> 16));
    v[6] = nr_one(v[6], (int)(o.w & 0xffffu)); v[7] = nr_one(v[7], (int)(o.w >> 16));
}

// A macroblock's |coefficient| values before they count (the final encode): every lane leaves its own in a 512-byte area of LDS, 16 bits each (a transform of
// 8-bit samples stays below 2^15), in the order of the lanes — 4x4 blocks: block (lane >> 2), raster index (lane & 3) * 4 + i; 8x8 blocks (lanes 0..31): block
// (lane >> 3), raster index (lane & 7) * 8 + i.  No cross-lane traffic and two or four registers at the site, where the transform's own registers are live; the
// sums per index are taken when the macroblock's type is known (nr_pend_sum), where nothing else is
template <int LANES>
__device__ __forceinline__ void nr_stash4(const int v[4], int lane, uint16_t *dst)
{
    static_assert(LANES == 32 || LANES == 64, "chroma (lanes 0..31) / luma");
    lane = relane(lane);
    uint2 o;
    o.x = (uint32_t)abs(v[0]) | ((uint32_t)abs(v[1]) << 16); o.y = (uint32_t)abs(v[2]) | ((uint32_t)abs(v[3]) << 16);
    if (LANES == 64 || lane < 32) *(uint2 *)(dst + lane * 4) = o;
}
__device__ __forceinline__ void nr_stash8(const int v[8], int lane, uint16_t *dst)
{
    lane = relane(lane);
    uint2 lo, hi;          // (two 8-byte stores: the area is 8-byte aligned)
    lo.x = (uint32_t)abs(v[0]) | ((uint32_t)abs(v[1]) << 16); lo.y = (uint32_t)abs(v[2]) | ((uint32_t)abs(v[3]) << 16);
    hi.x = (uint32_t)abs(v[4]) | ((uint32_t)abs(v[5]) << 16); hi.y = (uint32_t)abs(v[6]) | ((uint32_t)abs(v[7]) << 16);
    if (lane < 32) { *(uint2 *)(dst + lane * 8) = lo; *(uint2 *)(dst + lane * 8 + 4) = hi; }
}
// the sum at raster index e over nblk stashed blocks of n entries (<= 16 x 65535: no wrap)
__device__ __forceinline__ uint32_t nr_pend_sum(const uint16_t *pend, int e, int nblk, int n)
{
    uint32_t a = 0;
    for (int b = 0; b < nblk; b++) a += pend[b * n + e];
    return a;
}

}  // namespace x264gpu

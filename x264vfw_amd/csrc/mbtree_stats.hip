// mbtree_stats.hip — the macroblock-tree statistics file's number format on the device ([x264-upstream] common/mc.c mbtree_fix8_pack / mbtree_fix8_unpack): a
// picture's quantiser offsets (single floats, where the lookahead leaves them and the encoder reads them) to and from the file's big-endian 8.8 fixed-point words,
// so that 2 bytes a macroblock cross the bus and no float array does.  A unit of its own: no other code object changes with it.
#include "common.hip.h"

namespace {

// the product rounded on its own, as the C source reads (both factors here are powers of two: exact, but nothing is left to the compiler's flags)
__device__ __forceinline__ float f_mul(float a, float b) {
#pragma clang fp contract(off)
    return a * b; }

// x264: (int16_t)(src * 256.0f), then endian_fix16.  The C cast truncates toward zero and is undefined out of range; x264's SIMD versions saturate, which is the rule
// stated here, with NaN -> 0
__device__ __forceinline__ uint16_t fix8_pack(float x)
{
    const float v = f_mul(x, 256.0f);
    int i;
    if (!(v == v)) i = 0;
    else if (v >= 32767.0f) i = 32767;
    else if (v <= -32768.0f) i = -32768;
    else i = (int)v;          // in range: truncation toward zero
    const unsigned u = (unsigned)i & 0xffffu;
    return (uint16_t)((u >> 8) | ((u & 0xffu) << 8));
}
__device__ __forceinline__ float fix8_unpack(uint16_t w)
{
    const int16_t i = (int16_t)(uint16_t)((w >> 8) | ((w & 0xffu) << 8));
    return f_mul((float)i, 1.0f / 256.0f);
}

__global__ __launch_bounds__(256) void k_mbtree_pack(const float *__restrict__ src, int n, uint16_t *__restrict__ dst)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = fix8_pack(src[i]);
}
__global__ __launch_bounds__(256) void k_mbtree_unpack(const uint16_t *__restrict__ src, int n, float *__restrict__ dst)
{
    for (int i = blockIdx.x * blockDim.x + threadIdx.x; i < n; i += gridDim.x * blockDim.x) dst[i] = fix8_unpack(src[i]);
}

// a picture has at most 36 864 macroblocks: one element a thread up to 256 workgroups, the stride loop takes what a caller asks beyond that
inline unsigned grid_for(int n) { const int g = (n + 255) / 256; return (unsigned)(g < 256 ? g : 256); }

}  // namespace

extern "C" {

int x264gpu_mbtree_pack(const float *d_offsets, int n, uint16_t *d_out, void *stream)
{
    ARG_TRY(d_offsets && d_out && n > 0);
    hipLaunchKernelGGL(k_mbtree_pack, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, d_offsets, n, d_out);
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}

int x264gpu_mbtree_unpack(const uint16_t *d_in, int n, float *d_offsets, void *stream)
{
    ARG_TRY(d_in && d_offsets && n > 0);
    hipLaunchKernelGGL(k_mbtree_unpack, dim3(grid_for(n)), dim3(256), 0, (hipStream_t)stream, d_in, n, d_offsets);
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}

}  // extern "C"

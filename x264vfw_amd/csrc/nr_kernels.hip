// nr_kernels.hip — x264 --nr beside the macroblock loop: the state update between pictures (x264_noise_reduction_update, [x264-upstream] encoder/encoder.c), the
// sum of a picture's per-slice statistics, and the denoise function (nr.hip.h) as a primitive.
#include "common.hip.h"
#include "nr.hip.h"

using namespace x264gpu;

namespace {

// coef_weight2 of the transforms (FIX8; x264_dct4_weight2_tab / x264_dct8_weight2_tab), raster index: the numbers of the trellis search's distortion weights
__constant__ const uint16_t c_nr_w8[6] = { 256, 201, 656, 227, 410, 363 };          // by normAdjust8x8 class (class8)
__device__ __forceinline__ unsigned nr_weight2(int cat, int i)
{
    if (cat == 1) return c_nr_w8[class8(i >> 3, i & 7)];
    const int odd = ((i >> 2) & 1) + (i & 1);
    return odd == 0 ? 800u : odd == 1 ? 320u : 128u;
}

// one workgroup of 192 threads a stream: thread = category * 64 + index
__global__ __launch_bounds__(192) void k_nr_update(x264gpu_nr_offsets *off, x264gpu_nr_sums *state, const x264gpu_nr_sums *pic, int strength)
{
    const int s = blockIdx.x, t = threadIdx.x, cat = t >> 6, i = t & 63;
    x264gpu_nr_sums *st = state + s;
    const bool used = cat == 1 || i < 16;
    uint64_t sum = st->sum[cat][i];
    uint32_t cnt = st->count[cat];
    if (pic) { sum += pic[s].sum[cat][i]; cnt += pic[s].count[cat]; }
    if (cnt > (cat == 1 ? 1u << 16 : 1u << 18)) { sum >>= 1; cnt >>= 1; }
    __syncthreads();          // every thread has read its category's count before one of them writes it
    st->sum[cat][i] = used ? sum : 0;
    if (i == 0) st->count[cat] = cnt;
    uint64_t o = 0;
    if (used && i > 0) {
        o = ((uint64_t)(unsigned)strength * cnt + sum / 2) / (sum * nr_weight2(cat, i) / 256 + 1);
        if (o > 32767) o = 32767;
    }
    off[s].off[cat][i] = (uint16_t)o;
}

// a picture's statistics: the sum of its slices' rows, in 64 bits (one workgroup of 256 threads a stream)
__global__ __launch_bounds__(256) void k_nr_gather(const x264gpu_nr_sums *part, int slices, x264gpu_nr_sums *pic)
{
    const int s = blockIdx.x, t = threadIdx.x;
    const x264gpu_nr_sums *p = part + (size_t)s * slices;
    if (t < 192) {
        uint64_t a = 0;
        for (int sl = 0; sl < slices; sl++) a += p[sl].sum[t >> 6][t & 63];
        pic[s].sum[t >> 6][t & 63] = a;
    } else if (t < 196) {
        uint32_t a = 0;
        if (t < 195) for (int sl = 0; sl < slices; sl++) a += p[sl].count[t - 192];
        (&pic[s].count[0])[t - 192] = a;
    }
}

// the primitive: one wavefront walks the blocks in passes of the macroblock loop's layouts — sixteen 4x4 blocks (lane >> 2 = block, lane & 3 = row) or four
// 8x8 blocks (lanes 0..31: lane >> 3 = block, lane & 7 = row; lanes 32..63 hold copies, as in the loop)
__global__ __launch_bounds__(64) void k_denoise_blocks(int16_t *coefs, int nblk, int cat, const x264gpu_nr_offsets *off, x264gpu_nr_sums *out)
{
    __shared__ __attribute__((aligned(16))) uint16_t offs[NR_OFF_N];
    __shared__ __attribute__((aligned(16))) uint16_t pend[256];
    const int lane = threadIdx.x;
    if (lane < NR_OFF_N / 2) ((uint32_t *)offs)[lane] = ((const uint32_t *)off)[nr_stage_src(lane)];
    lds_order();
    uint64_t acc = 0;          // lane i: the sum at index i
    if (cat == 1) {
        const int row = lane & 7;
        for (int b0 = 0; b0 < nblk; b0 += 4) {
            const int blk = b0 + ((lane >> 3) & 3);
            const bool valid = blk < nblk;
            int v[8];
#pragma unroll
            for (int i = 0; i < 8; i++) v[i] = valid ? coefs[(size_t)blk * 64 + row * 8 + i] : 0;
            lds_order();
            nr_stash8(v, lane, pend);
            nr_denoise8(v, offs + NR_O8, lane);
            lds_order();
            acc += nr_pend_sum(pend, lane, 4, 64);
            if (valid && lane < 32)
#pragma unroll
                for (int i = 0; i < 8; i++) coefs[(size_t)blk * 64 + row * 8 + i] = (int16_t)v[i];
        }
    } else {
        const int j = lane & 3;
        for (int b0 = 0; b0 < nblk; b0 += 16) {
            const int blk = b0 + (lane >> 2);
            const bool valid = blk < nblk;
            int v[4];
#pragma unroll
            for (int i = 0; i < 4; i++) v[i] = valid ? coefs[(size_t)blk * 16 + j * 4 + i] : 0;
            lds_order();
            nr_stash4<64>(v, lane, pend);
            nr_denoise4(v, offs + (cat ? NR_OC : NR_O4), lane);
            lds_order();
            if (lane < 16) acc += nr_pend_sum(pend, lane, 16, 16);
            if (valid)
#pragma unroll
                for (int i = 0; i < 4; i++) coefs[(size_t)blk * 16 + j * 4 + i] = (int16_t)v[i];
        }
    }
    if (out) {
        for (int c = 0; c < 3; c++) out->sum[c][lane] = c == cat ? acc : 0;
        if (lane < 4) (&out->count[0])[lane] = lane == cat ? (uint32_t)nblk : 0u;
    }
}

}  // namespace

namespace x264gpu {
void launch_nr_gather(const x264gpu_nr_sums *part, int slices, x264gpu_nr_sums *pic, int streams, hipStream_t st)
{
    hipLaunchKernelGGL(k_nr_gather, dim3(streams), dim3(256), 0, st, part, slices, pic);
}
}

extern "C" {

int x264gpu_nr_update(x264gpu_nr_offsets *d_off, x264gpu_nr_sums *d_state, const x264gpu_nr_sums *d_pic, int streams, int strength, void *stream)
{
    ARG_TRY(d_off && d_state && streams >= 1 && strength >= 0 && strength <= 65536);
    hipLaunchKernelGGL(k_nr_update, dim3(streams), dim3(192), 0, (hipStream_t)stream, d_off, d_state, d_pic, strength);
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}

int x264gpu_denoise_blocks(int16_t *d_coefs, int nblk, int cat, const x264gpu_nr_offsets *d_off, x264gpu_nr_sums *d_out, void *stream)
{
    ARG_TRY(d_coefs && d_off && nblk >= 1 && cat >= 0 && cat <= 2);
    hipLaunchKernelGGL(k_denoise_blocks, dim3(1), dim3(64), 0, (hipStream_t)stream, d_coefs, nblk, cat, d_off, d_out);
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}

}  // extern "C"

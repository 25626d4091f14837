// quality.hip — per-picture quality statistics (x264 --psnr / --ssim: [x264-upstream] common/pixel.c pixel_ssd_wxh, pixel_ssim_wxh, ssim_end1 for 8-bit
// samples, restated): the exact sum of squared differences of every plane and the sum of x264's SSIM window values over luma, for n picture pairs in one pass.
//
// One load of a and b serves both statistics.  A CELL is 4 x 4 luma samples of the grid whose origin is (2, 2) — x264 offsets its SSIM blocks by 2 so that the
// windows do not sit on transform blocks — extended by one cell to the left / top so that the cells tile the whole picture (edge cells are clipped: bytes outside
// the picture read as 0 in a AND b).  A lane owns a column of cells over a band of QL_ROWS cell rows: per cell the four sums s1 = sum a, s2 = sum b,
// ss = sum (a^2 + b^2), s12 = sum ab from v_sad_u8 / v_dot4_u32_u8 on the packed dwords; SSD = ss - 2 s12; an SSIM window = the cell with its lower neighbour (kept
// in registers) and the pair to the right (the next lane: a wave is 63 owned columns and one of overlap; a band reads one cell row of overlap).
// Workgroup partials go to a slab; k_quality_sum adds them per picture in a fixed order: no float atomics, bit-identical from run to run.
// Samples are fetched as ALIGNED dwords joined by v_alignbyte_b32, whatever the alignment of a row (tight I420 of odd chroma width included); an aligned dword
// is read only if it holds a sample of the picture, so nothing outside the caller's buffers is touched.
#include "quality.hip.h"
#include <map>
#include <mutex>
#include <utility>

namespace x264gpu {

constexpr int QL_ROWS = 16;      // luma: cell rows a workgroup owns (+ 1 of overlap)
constexpr int QL_COLS = 63;      // ... cell columns a wave owns (+ 1 of overlap)
constexpr int QC_ROWS = 32;      // chroma: sample rows a workgroup owns

struct QPart { unsigned long long ssd; double ssim; };

// the 4 bytes at p (any alignment), of which bytes [v0, v1) are samples of the picture (0 <= v0 < v1 <= 4); the others come back 0
__device__ __forceinline__ uint32_t ld4(const uint8_t *p, int v0, int v1)
{
    const uintptr_t ad = (uintptr_t)p;
    const int sh = (int)(ad & 3);
    const uint32_t *q = (const uint32_t *)(ad - (uintptr_t)sh);
    uint32_t lo = 0, hi = 0;
    if (v0 < 4 - sh) lo = q[0];
    if (v1 > 4 - sh) hi = q[1];
    const uint32_t v = __builtin_amdgcn_alignbyte(hi, lo, (uint32_t)sh);
    return v & (0xffffffffu >> (8 * (4 - v1))) & (0xffffffffu << (8 * v0));
}

__device__ __forceinline__ uint32_t dot4(uint32_t a, uint32_t b) { return __builtin_amdgcn_udot4(a, b, 0u, false); }
__device__ __forceinline__ uint32_t sum4(uint32_t a) { return __builtin_amdgcn_sad_u8(a, 0u, 0u); }

// x264's ssim_end1 for 8-bit samples: 32-bit integers, the quotient in single floats
__device__ __forceinline__ float ssim_end1(int s1, int s2, int ss, int s12)
{
    const int c1 = 416, c2 = 235963;            // (int)(.01^2 * 255^2 * 64 + .5), (int)(.03^2 * 255^2 * 64 * 63 + .5)
    const int vars = ss * 64 - s1 * s1 - s2 * s2, covar = s12 * 64 - s1 * s2;
    return (float)(2 * s1 * s2 + c1) * (float)(2 * covar + c2) / ((float)(s1 * s1 + s2 * s2 + c1) * (float)(vars + c2));
}

__device__ __forceinline__ unsigned long long wave_sum(unsigned long long v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);
    return v;
}
__device__ __forceinline__ double wave_sum(double v)
{
#pragma unroll
    for (int d = 32; d; d >>= 1) v += __shfl_xor(v, d);          // a fixed tree: the same bits every run
    return v;
}

static inline int ql_parts_x(int w) { const int ecols = (w + 5) >> 2; return ((ecols + QL_COLS - 1) / QL_COLS + 3) / 4; }
static inline int ql_parts_y(int h) { const int erows = (h + 5) >> 2; return (erows + QL_ROWS - 1) / QL_ROWS; }
static inline int qc_parts_x(int w, int step) { return ((w / 2 * step + 3) / 4 + 255) / 256; }
static inline int qc_parts_y(int h) { return (h / 2 + QC_ROWS - 1) / QC_ROWS; }

// grid (ql_parts_x, ql_parts_y, n) x 256: wave wv of workgroup bx owns cell columns [(4 bx + wv) * 63, + 63)
__global__ __launch_bounds__(256) void k_quality_luma(QPlanes q, QPart *__restrict__ slab)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6, s = blockIdx.z;
    const int ec = (blockIdx.x * 4 + wv) * QL_COLS + lane;
    const int ecols = (q.w + 5) >> 2, erows = (q.h + 5) >> 2, zc = (q.w - 2) >> 2, zr = (q.h - 2) >> 2;
    const uint8_t *pa = q.a_y + (size_t)s * q.a_pitch_y, *pb = q.b_y + (size_t)s * q.b_pitch_y;
    const int x0 = 4 * ec - 2;
    const int v0 = x0 < 0 ? -x0 : 0, v1 = q.w - x0 < 4 ? q.w - x0 : 4;
    const bool col_in = ec < ecols, own_col = col_in && lane < QL_COLS;
    const bool win_col = lane < QL_COLS && ec >= 1 && ec - 1 < zc - 1;          // window column c = ec - 1: blocks c, c + 1 of [0, zc)
    const int er0 = blockIdx.y * QL_ROWS, er1 = min(er0 + QL_ROWS, erows), er_end = min(er1 + 1, erows);
    uint32_t ssd = 0;
    double acc = 0.0;
    int p1 = 0, p2 = 0, pss = 0, p12 = 0;
    for (int er = er0; er < er_end; er++) {
        int s1 = 0, s2 = 0, ss = 0, s12 = 0;
        if (col_in) {
#pragma unroll
            for (int j = 0; j < 4; j++) {
                const int y = 4 * er - 2 + j;
                if (y >= 0 && y < q.h) {
                    const uint32_t a = ld4(pa + (ptrdiff_t)y * q.a_sy + x0, v0, v1), b = ld4(pb + (ptrdiff_t)y * q.b_sy + x0, v0, v1);
                    s1 += (int)sum4(a); s2 += (int)sum4(b); ss += (int)(dot4(a, a) + dot4(b, b)); s12 += (int)dot4(a, b);
                }
            }
        }
        if (er < er1 && own_col) ssd += (uint32_t)(ss - 2 * s12);          // <= 17 cells x 16 x 255^2 a lane
        // the window whose upper blocks are cell row er - 1 (block row er - 2 of [0, zr)): this band's if it owns that row
        const int t1 = p1 + s1, t2 = p2 + s2, tss = pss + ss, t12 = p12 + s12;
        const int n1 = __shfl_down(t1, 1), n2 = __shfl_down(t2, 1), nss = __shfl_down(tss, 1), n12 = __shfl_down(t12, 1);
        if (er > er0 && er >= 2 && er - 2 < zr - 1 && win_col) acc += (double)ssim_end1(t1 + n1, t2 + n2, tss + nss, t12 + n12);
        p1 = s1; p2 = s2; pss = ss; p12 = s12;
    }
    __shared__ QPart part[4];
    const unsigned long long wssd = wave_sum((unsigned long long)ssd);
    const double wacc = wave_sum(acc);
    if (lane == 0) { part[wv].ssd = wssd; part[wv].ssim = wacc; }
    __syncthreads();
    if (threadIdx.x == 0) {
        QPart r = part[0];
        for (int i = 1; i < 4; i++) { r.ssd += part[i].ssd; r.ssim += part[i].ssim; }
        slab[((size_t)s * gridDim.y + blockIdx.y) * gridDim.x + blockIdx.x] = r;
    }
}

// SSD of the chroma planes.  STEP 1: grid (qc_parts_x, qc_parts_y, 2 n), z = pair * 2 + plane; STEP 2 (interleaved U, V): grid (.., .., n), both planes at once.
// slab[(pair * 2 + plane) * parts + by * gridDim.x + bx]
template <int STEP> __global__ __launch_bounds__(256) void k_quality_chroma(QPlanes q, unsigned long long *__restrict__ slab)
{
    const int lane = threadIdx.x & 63, wv = threadIdx.x >> 6;
    const int s = STEP == 2 ? blockIdx.z : blockIdx.z >> 1, pl = STEP == 2 ? 0 : blockIdx.z & 1;
    const int wb = (q.w >> 1) * STEP, rows = q.h >> 1;
    const int x0 = 4 * (blockIdx.x * 256 + threadIdx.x);
    const int v1 = wb - x0 < 4 ? wb - x0 : 4;
    const uint8_t *pa = q.a_c + (size_t)s * q.a_pitch_c + (pl ? q.a_voff : 0) + x0, *pb = q.b_c + (size_t)s * q.b_pitch_c + (pl ? q.b_voff : 0) + x0;
    const int r0 = blockIdx.y * QC_ROWS, r1 = min(r0 + QC_ROWS, rows);
    uint32_t d0 = 0, d1 = 0;          // <= 32 rows x 4 x 255^2 a lane
    if (v1 > 0) {
#pragma unroll 4
        for (int y = r0; y < r1; y++) {
            const uint32_t a = ld4(pa + (ptrdiff_t)y * q.a_sc, 0, v1), b = ld4(pb + (ptrdiff_t)y * q.b_sc, 0, v1);
            if (STEP == 1) d0 += dot4(a, a) + dot4(b, b) - 2 * dot4(a, b);
            else {
                const uint32_t au = a & 0x00ff00ffu, av = (a >> 8) & 0x00ff00ffu, bu = b & 0x00ff00ffu, bv = (b >> 8) & 0x00ff00ffu;
                d0 += dot4(au, au) + dot4(bu, bu) - 2 * dot4(au, bu);
                d1 += dot4(av, av) + dot4(bv, bv) - 2 * dot4(av, bv);
            }
        }
    }
    __shared__ unsigned long long part[4][2];
    const unsigned long long w0 = wave_sum((unsigned long long)d0), w1 = STEP == 2 ? wave_sum((unsigned long long)d1) : 0ull;
    if (lane == 0) { part[wv][0] = w0; part[wv][1] = w1; }
    __syncthreads();
    if (threadIdx.x == 0) {
        const size_t parts = (size_t)gridDim.x * gridDim.y, at = (size_t)blockIdx.y * gridDim.x + blockIdx.x;
        slab[((size_t)s * 2 + pl) * parts + at] = part[0][0] + part[1][0] + part[2][0] + part[3][0];
        if (STEP == 2) slab[((size_t)s * 2 + 1) * parts + at] = part[0][1] + part[1][1] + part[2][1] + part[3][1];
    }
}

// one thread per picture pair: the partials in slab order
__global__ __launch_bounds__(64) void k_quality_sum(const QPart *__restrict__ lslab, int lparts, const unsigned long long *__restrict__ cslab, int cparts, int n, int flags,
                                                    uint32_t cnt, x264gpu_quality *__restrict__ out)
{
    const int s = blockIdx.x * 64 + threadIdx.x;
    if (s >= n) return;
    x264gpu_quality r;
    r.ssd[0] = r.ssd[1] = r.ssd[2] = 0; r.ssim_sum = 0.0; r.ssim_cnt = 0; r.pad = 0;
    unsigned long long y = 0; double m = 0.0;
    for (int i = 0; i < lparts; i++) { y += lslab[(size_t)s * lparts + i].ssd; m += lslab[(size_t)s * lparts + i].ssim; }
    if (flags & X264GPU_QUALITY_PSNR) {
        r.ssd[0] = y;
        for (int p = 0; p < 2; p++) { unsigned long long c = 0; for (int i = 0; i < cparts; i++) c += cslab[((size_t)s * 2 + p) * cparts + i]; r.ssd[1 + p] = c; }
    }
    if (flags & X264GPU_QUALITY_SSIM) { r.ssim_sum = m; r.ssim_cnt = cnt; }
    out[s] = r;
}

size_t quality_slab_bytes(int n, int w, int h)
{
    // chroma: the larger of the two layouts' workgroup counts
    const int cp = (qc_parts_x(w, 2) > qc_parts_x(w, 1) ? qc_parts_x(w, 2) : qc_parts_x(w, 1)) * qc_parts_y(h);
    return (size_t)n * ((size_t)ql_parts_x(w) * ql_parts_y(h) * sizeof(QPart) + (size_t)2 * cp * sizeof(unsigned long long));
}

int launch_quality(const QPlanes &q, int n, int flags, void *slab, x264gpu_quality *d_out, hipStream_t st)
{
    const int lx = ql_parts_x(q.w), ly = ql_parts_y(q.h), cx = qc_parts_x(q.w, q.step), cy = qc_parts_y(q.h);
    QPart *lslab = (QPart *)slab;
    unsigned long long *cslab = (unsigned long long *)(lslab + (size_t)n * lx * ly);
    hipLaunchKernelGGL(k_quality_luma, dim3(lx, ly, n), dim3(256), 0, st, q, lslab);
    if (flags & X264GPU_QUALITY_PSNR) {
        if (q.step == 2) hipLaunchKernelGGL(k_quality_chroma<2>, dim3(cx, cy, n), dim3(256), 0, st, q, cslab);
        else hipLaunchKernelGGL(k_quality_chroma<1>, dim3(cx, cy, 2 * n), dim3(256), 0, st, q, cslab);
    }
    const int zc = (q.w - 2) >> 2, zr = (q.h - 2) >> 2;
    hipLaunchKernelGGL(k_quality_sum, dim3((n + 63) / 64), dim3(64), 0, st, lslab, lx * ly, cslab, cx * cy, n, flags, (uint32_t)((zc - 1) * (zr - 1)), d_out);
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}

// the primitive has no context to keep its slab in: one per (device, stream), grown on demand, kept while the library is loaded.  Calls on one stream run in order,
// so they can share theirs; growing frees the old one, which waits for the device.
static int primitive_slab(hipStream_t st, size_t bytes, void **out)
{
    static std::mutex mu;
    static std::map<std::pair<int, void *>, std::pair<void *, size_t>> slabs;
    int dev = 0;
    HIP_TRY(hipGetDevice(&dev));
    std::lock_guard<std::mutex> lock(mu);
    std::pair<void *, size_t> &sl = slabs[std::make_pair(dev, (void *)st)];
    if (sl.second < bytes) {
        if (sl.first) HIP_TRY(hipFree(sl.first));
        sl.first = nullptr; sl.second = 0;
        hipError_t e = hipMalloc(&sl.first, bytes);
        if (e != hipSuccess) { sl.first = nullptr; return set_err(e == hipErrorOutOfMemory ? X264GPU_ENOMEM : X264GPU_EHIP, "quality slab", e); }
        sl.second = bytes;
    }
    *out = sl.first;
    return X264GPU_OK;
}

}  // namespace x264gpu
using namespace x264gpu;

extern "C" int x264gpu_picture_quality(const uint8_t *d_a, const uint8_t *d_b, int n, int w, int h, int flags, x264gpu_quality *d_out, void *stream)
{
    ARG_TRY(d_a && d_b && d_out && n >= 1 && n <= 32767);
    ARG_TRY(flags >= 1 && flags <= 3 && w >= 16 && h >= 16 && !(w & 1) && !(h & 1) && w <= 16384 && h <= 16384);
    void *slab = nullptr;
    const int rc = primitive_slab((hipStream_t)stream, quality_slab_bytes(n, w, h), &slab);
    if (rc != X264GPU_OK) return rc;
    const size_t pic = (size_t)w * h * 3 / 2, csz = (size_t)(w / 2) * (h / 2);
    QPlanes q;
    q.a_y = d_a; q.b_y = d_b; q.a_c = d_a + (size_t)w * h; q.b_c = d_b + (size_t)w * h;
    q.a_pitch_y = q.b_pitch_y = q.a_pitch_c = q.b_pitch_c = pic; q.a_voff = q.b_voff = csz;
    q.a_sy = q.b_sy = w; q.a_sc = q.b_sc = w / 2;
    q.w = w; q.h = h; q.step = 1;
    return launch_quality(q, n, flags, slab, d_out, (hipStream_t)stream);
}

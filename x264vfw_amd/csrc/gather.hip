// gather.hip — x264gpu_gather_rows: rows that lie anywhere in device memory, copied into one contiguous [rows][row_bytes] array in one launch.
// The host's cross-session batcher (host/batch.cpp) builds the [streams][mb_count] quantiser offsets and the [streams][mb_count][2] lookahead vectors of a round from
// its members' own arrays with it: one launch an array instead of one runtime call a member.  Memory streaming and nothing else: no LDS, no atomics, plain stores.
#include "common.hip.h"

using namespace x264gpu;

namespace {

constexpr int GATHER_THREADS = 256, GATHER_VPT = 2;                  // 16-byte vectors a thread: both loads are issued before the first store
constexpr int GATHER_VPC = GATHER_THREADS * GATHER_VPT;              // vectors a block: 8 KiB of a row

// how a 16-byte piece of the source is read once the DESTINATION is 16-aligned: the source sits at the same offset within 16 bytes (one vector load), at a multiple
// of four from it (four dwords), or anywhere (sixteen bytes).  No load leaves [src, src + row_bytes)
enum { G_ZERO, G_VEC, G_DWORD, G_BYTE };
// a row pointer read from the table is a pointer into device memory: said so, or the compiler reads through it with flat loads
#define GATHER_GLOBAL __attribute__((address_space(1)))
typedef const GATHER_GLOBAL uint8_t *gather_src;
typedef uint32_t gather_u32x4 __attribute__((ext_vector_type(4)));

template<int MODE> __device__ __forceinline__ uint4 gather_load(gather_src p)
{
    if (MODE == G_ZERO) return make_uint4(0, 0, 0, 0);
    if (MODE == G_VEC) { const gather_u32x4 v = *(const GATHER_GLOBAL gather_u32x4 *)p; return make_uint4(v.x, v.y, v.z, v.w); }
    if (MODE == G_DWORD) { const GATHER_GLOBAL uint32_t *q = (const GATHER_GLOBAL uint32_t *)p; return make_uint4(q[0], q[1], q[2], q[3]); }
    uint32_t w[4];
#pragma unroll
    for (int i = 0; i < 4; i++) w[i] = (uint32_t)p[4 * i] | (uint32_t)p[4 * i + 1] << 8 | (uint32_t)p[4 * i + 2] << 16 | (uint32_t)p[4 * i + 3] << 24;
    return make_uint4(w[0], w[1], w[2], w[3]);
}

// vectors [v0, v0 + GATHER_VPC) of the row's aligned middle (nv vectors from s / o16)
template<int MODE> __device__ __forceinline__ void gather_body(gather_src s, uint4 *o16, size_t v0, size_t nv, int t)
{
    uint4 v[GATHER_VPT];
#pragma unroll
    for (int i = 0; i < GATHER_VPT; i++) { const size_t idx = v0 + (size_t)(i * GATHER_THREADS + t); if (idx < nv) v[i] = gather_load<MODE>(s + (idx << 4)); }
#pragma unroll
    for (int i = 0; i < GATHER_VPT; i++) { const size_t idx = v0 + (size_t)(i * GATHER_THREADS + t); if (idx < nv) o16[idx] = v[i]; }
}

// grid (chunks, rows): block (c, r) copies vectors [c * GATHER_VPC, ...) of row row0 + r; block (0, r) also the row's ends, at most 15 bytes each
__global__ __launch_bounds__(GATHER_THREADS) void k_gather_rows(const void *const *rows, size_t row_bytes, uint8_t *dst, int row0)
{
    const int r = row0 + (int)blockIdx.y, t = threadIdx.x;
    // the row's base is one value a block: into scalar registers, so that the branches below are uniform and the addresses are scalar base + lane offset
    const uintptr_t sp = (uintptr_t)rows[r];
    const gather_src src = (gather_src)((uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)sp) |
                                           (uintptr_t)(uint32_t)__builtin_amdgcn_readfirstlane((int)(uint32_t)(sp >> 32)) << 32);
    uint8_t *out = dst + (size_t)r * row_bytes;
    const size_t to_al = (size_t)(-(uintptr_t)out & 15), head = to_al < row_bytes ? to_al : row_bytes;
    const size_t nv = (row_bytes - head) >> 4, tail_at = head + (nv << 4), tail = row_bytes - tail_at;
    if (blockIdx.x == 0) {
        if ((size_t)t < head) out[t] = src ? src[t] : (uint8_t)0;
        else if (t >= 16 && (size_t)(t - 16) < tail) out[tail_at + (size_t)(t - 16)] = src ? src[tail_at + (size_t)(t - 16)] : (uint8_t)0;
    }
    const size_t v0 = (size_t)blockIdx.x * GATHER_VPC;
    if (v0 >= nv) return;
    uint4 *o16 = (uint4 *)(out + head);
    const gather_src s = src + head;
    const unsigned delta = (unsigned)(((uintptr_t)s - (uintptr_t)o16) & 15);
    if (!src) gather_body<G_ZERO>(s, o16, v0, nv, t);
    else if (delta == 0) gather_body<G_VEC>(s, o16, v0, nv, t);
    else if ((delta & 3) == 0) gather_body<G_DWORD>(s, o16, v0, nv, t);
    else gather_body<G_BYTE>(s, o16, v0, nv, t);
}

}  // namespace

extern "C" {

int x264gpu_gather_rows(const void *const *d_rows, size_t row_bytes, void *d_dst, int rows, void *stream)
{
    ARG_TRY(d_rows && d_dst && rows >= 1 && row_bytes > 0);
    const size_t chunks = (row_bytes >> 4) / GATHER_VPC + 1;
    ARG_TRY(chunks <= 0x7fffffffu);
    for (int row0 = 0; row0 < rows; row0 += 65535) {          // (a grid's second dimension holds 65535 blocks)
        const int n = rows - row0 < 65535 ? rows - row0 : 65535;
        hipLaunchKernelGGL(k_gather_rows, dim3((unsigned)chunks, (unsigned)n), dim3(GATHER_THREADS), 0, (hipStream_t)stream, d_rows, row_bytes, (uint8_t *)d_dst, row0);
    }
    HIP_TRY(hipGetLastError());
    return X264GPU_OK;
}

}  // extern "C"

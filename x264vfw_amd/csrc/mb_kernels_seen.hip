// mb_kernels_seen.hip — which instantiations of the macroblock loop (k_mb.hip.h k_mb_slice<M, ME, PS, RD, BS, PSY, NR>) this process has launched: host code only.
// mb_launch notes the id of every launch here; x264gpu_mb_kernels_seen hands the distinct ids out, so that a test proves which compiled kernel it ran
// (tests/test_gpu_mb_instantiations.py).  A launch of an id already noted costs one load of its bit; a new id is appended under the mutex.
#include "common.hip.h"
#include <atomic>
#include <mutex>

namespace x264gpu {
namespace {
constexpr int MB_IDS_MAX = 256;                     // (the tree instantiates 103 + 5 with QP-RD + 38 of x264gpu_encoder_set_nr_any)
std::atomic<uint32_t> g_bits[4 * 65536 / 32];       // bit id: noted since the last reset (bit 16 of an id: the QP-RD instantiation of the tuple, mb_launch_qprd; bit 17: mb_launch_nr_any)
uint32_t g_ids[MB_IDS_MAX];                         // the ids in the order of their first launch
int g_n;
std::mutex g_mu;
}  // namespace

void mb_kernel_note(uint32_t id)
{
    id &= 0x3ffff;
    if (g_bits[id >> 5].load(std::memory_order_relaxed) >> (id & 31) & 1) return;
    std::lock_guard<std::mutex> lock(g_mu);
    if (g_bits[id >> 5].load(std::memory_order_relaxed) >> (id & 31) & 1) return;
    if (g_n < MB_IDS_MAX) g_ids[g_n++] = id;
    g_bits[id >> 5].fetch_or(1u << (id & 31), std::memory_order_relaxed);
}
}  // namespace x264gpu
using namespace x264gpu;

extern "C" int x264gpu_mb_kernels_seen(uint32_t *ids, int max, int reset)
{
    std::lock_guard<std::mutex> lock(g_mu);
    const int n = g_n;
    for (int i = 0; i < n && i < max && ids; i++) ids[i] = g_ids[i];
    if (reset) {
        for (int i = 0; i < n; i++) g_bits[g_ids[i] >> 5].store(0, std::memory_order_relaxed);
        g_n = 0;
    }
    return n;
}

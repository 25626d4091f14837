// siderows.cpp — siderows.hpp has the contract
#include "siderows.hpp"

// The gather entry is resolved weakly: with a device library without it (an older build; the tests' CPU stand-in) the rows are copied one by one instead.
#pragma weak x264gpu_gather_rows

namespace x264host {

int16_t *side_rows_absent(size_t nmb)
{
    int16_t *d = nullptr;
    const int16_t absent = 0x7fff;
    if (x264gpu_malloc((void **)&d, nmb * 4) == X264GPU_OK && x264gpu_memset(d, 0, nmb * 4, nullptr) == X264GPU_OK &&
        x264gpu_stream_sync(nullptr) == X264GPU_OK && x264gpu_memcpy_h2d(d, &absent, sizeof(absent), nullptr) == X264GPU_OK) return d;
    if (d) x264gpu_free(d);
    return nullptr;
}

bool side_rows_gather(const void *const *tab, const bool any[3], const void **d_tab, uint8_t *const d_dst[3], size_t N, size_t row, void *st, void *tab_stream)
{
    bool ok = true;
    if (x264gpu_gather_rows) {
        // the table goes up on a stream of its own where there is one, not on the compute stream: x264gpu_memcpy_h2d waits for its stream
        ok = x264gpu_memcpy_h2d((void *)d_tab, tab, 3 * N * sizeof(void *), tab_stream) == X264GPU_OK;
        for (int a = 0; a < 3 && ok; a++) if (any[a]) ok = x264gpu_gather_rows(d_tab + (size_t)a * N, row, d_dst[a], (int)N, st) == X264GPU_OK;
    } else
        for (int a = 0; a < 3 && ok; a++) if (any[a]) for (size_t s = 0; s < N && ok; s++) {
            const void *src = tab[(size_t)a * N + s];
            ok = (src ? x264gpu_memcpy_d2d(d_dst[a] + s * row, src, row, st) : x264gpu_memset(d_dst[a] + s * row, 0, row, st)) == X264GPU_OK;
        }
    return ok;
}

}  // namespace x264host

// quality.hip.h — the picture-quality pass (quality.hip) as the two entries of include/x264gpu.h see it: one description of `n` picture pairs and one launcher.
#pragma once
#include "common.hip.h"

namespace x264gpu {

// `n` pairs of pictures a / b, pair s at base + s * pitch.  Luma: rows of w samples.  Chroma, step 1: two planes of (w/2) x (h/2) samples, V `voff` bytes behind U;
// step 2: one plane of interleaved U, V pairs (NV12), w bytes a row.  Any alignment; only the visible w x h samples are read.
struct QPlanes {
    const uint8_t *a_y, *b_y, *a_c, *b_c;
    size_t a_pitch_y, b_pitch_y, a_pitch_c, b_pitch_c, a_voff, b_voff;
    int a_sy, b_sy, a_sc, b_sc;          // row strides in bytes
    int w, h, step;
};
size_t quality_slab_bytes(int n, int w, int h);
// queues the pass on `st`: partial sums per workgroup into `slab` (quality_slab_bytes), then their sum in a fixed order into d_out[n]
int launch_quality(const QPlanes &q, int n, int flags, void *slab, x264gpu_quality *d_out, hipStream_t st);

}  // namespace x264gpu

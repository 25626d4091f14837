// mb_slice_nr_b_umh.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction (x264gpu_encoder_set_nr: the NR instantiations, which denoise every inter
// residual they transform with the stream's offsets and gather the statistics of the final encodes), B slices under --me umh: analysed without RD (RD 7), with RD and trellis 1 (RD 3) or trellis 2 (RD 4); a translation unit of its own so
// that the instantiations build in parallel.  The selection mirrors the psy units'.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_nr_b_umh(const EncK &k, int streams, hipStream_t st)
{
    if (k.subme < 7) mb_launch<2, 2, true, 7, true, false, true>(k, streams, st);
    else if (k.trellis & 64) mb_launch<2, 2, true, 4, true, false, true>(k, streams, st);
    else mb_launch<2, 2, true, 3, true, false, true>(k, streams, st);
}
}  // namespace x264gpu

// mb_slice_nr_umh.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction (x264gpu_encoder_set_nr: the NR instantiations, which denoise every inter
// residual they transform with the stream's offsets and gather the statistics of the final encodes), P slices under --me umh, trellis 1 (RD 3) and trellis 2 (RD 4); a translation unit of its own so
// that the instantiations build in parallel.  The selection mirrors the psy units'.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_nr_umh(const EncK &k, int streams, hipStream_t st)
{
    if (k.trellis & 64) mb_launch<2, 2, true, 4, false, false, true>(k, streams, st);
    else mb_launch<2, 2, true, 3, false, false, true>(k, streams, st);
}
}  // namespace x264gpu

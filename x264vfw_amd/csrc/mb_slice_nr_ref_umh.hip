// mb_slice_nr_ref_umh.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction (x264gpu_encoder_set_nr: the NR instantiations, which denoise every inter
// residual they transform with the stream's offsets and gather the statistics of the final encodes), P slices under --me umh at --subme 8 and up (RD refinement), trellis 1 (RD 5) and trellis 2 (RD 6); a translation unit of its own so
// that the instantiations build in parallel.  The selection mirrors the psy units'.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_nr_ref_umh(const EncK &k, int streams, hipStream_t st)
{
    if (k.trellis & 64) mb_launch<5, 2, true, 6, false, false, true>(k, streams, st);
    else mb_launch<5, 2, true, 5, false, false, true>(k, streams, st);
}
}  // namespace x264gpu

// mb_slice_psy_ref_hex.hip — the macroblock-loop kernel (k_mb.hip.h) with psy-trellis (cfg.psy_trellis_q8 != 0: the PSY instantiations, which hold the
// source transform of every macroblock and run the psy variant of the trellis search at the luma sites), P slices under --me hex with RD refinement (--subme 8 and up), trellis 1 (RD 5) and trellis 2 (RD 6); a translation unit of its own so
// that the instantiations build in parallel.  The selection mirrors the plain units'.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_psy_ref_hex(const EncK &k, int streams, hipStream_t st)
{
    if (k.trellis & 64) mb_launch<5, 1, true, 6, false, true>(k, streams, st);
    else mb_launch<5, 1, true, 5, false, true>(k, streams, st);
}
}  // namespace x264gpu

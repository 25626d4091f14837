// mb_slice_hex.hip — the macroblock-loop kernel (k_mb.hip.h) instantiated for --me hex: one translation unit per search method so that
// the four instantiation pairs build in parallel.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_ref_hex(const EncK &k, int streams, hipStream_t st);        // mb_slice_ref_hex.hip
void launch_mb_slice_hex(const EncK &k, int streams, bool big_margin, hipStream_t st)
{
    if (k.rd && k.cabac && (((k.rd >> 1) & 63) || k.subme >= 8)) { launch_mb_slice_ref_hex(k, streams, st); return; }      // --subme 8 and up: the +-5 sample sub-pel neighbourhood, RD refinement of the sites cfg.rd names
    if (k.rd && k.cabac && (k.trellis & 64)) mb_launch<2, 1, true, 4>(k, streams, st);      // ... --trellis 2
    else if (k.rd && k.cabac && k.trellis) mb_launch<2, 1, true, 3>(k, streams, st);      // ... and trellis
    else if (k.rd && k.cabac) mb_launch<2, 1, true, 2>(k, streams, st);      // ... with CABAC sizes
    else if (k.rd) mb_launch<2, 1, true, 1>(k, streams, st);      // RD: subme 6 / 7, the +-2 sub-pel neighbourhood
    else if (big_margin) mb_launch<5, 1, true>(k, streams, st);
    else mb_launch<2, 1, true>(k, streams, st);
}
}  // namespace x264gpu

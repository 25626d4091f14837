// mb_slice_b.hip — the macroblock-loop kernel (k_mb.hip.h) instantiated for B slices (--me hex; RD sessions with CABAC, without the trellis quantiser,
// with it in the final encode, and with it in the analysis too): a translation unit of its own, like the per-method ones (mb_slice_b_dia / _umh / _esa.hip).
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_ref_b_hex(const EncK &k, int streams, hipStream_t st);        // mb_slice_ref_b_hex.hip
void launch_mb_slice_b1_hex(const EncK &k, int streams, hipStream_t st);        // mb_slice_b1_hex.hip
void launch_mb_slice_b0_hex(const EncK &k, int streams, hipStream_t st);        // mb_slice_b0_hex.hip
void launch_mb_slice_b_hex(const EncK &k, int streams, hipStream_t st)
{
    if (!k.rd || k.subme < 7) { launch_mb_slice_b0_hex(k, streams, st); return; }
    if (!k.cabac) { launch_mb_slice_b1_hex(k, streams, st); return; }      // RD with CAVLC bit counts
    if (k.cabac && (k.subme >= 9 || (k.rd & 64))) { launch_mb_slice_ref_b_hex(k, streams, st); return; }      // --subme 9: the +-5 sample sub-pel neighbourhood (4 + 10 iterations) and RD refinement of the sites cfg.rd names
    if (k.trellis & 64) mb_launch<2, 1, true, 4, true>(k, streams, st);      // --trellis 2
    else if (k.trellis) mb_launch<2, 1, true, 3, true>(k, streams, st);
    else mb_launch<2, 1, true, 2, true>(k, streams, st);
}
}  // namespace x264gpu

// nr_any_slice_b_hex.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction in the toolsets x264gpu_encoder_set_nr_any adds, B slices under --me hex:
// analysed without RD (k_mb_b.inc's RD == 0 branches), RD with CAVLC bit counts, RD with CABAC sizes; a translation unit of its own.
// (Not mb_slice_*.hip, not mb_launch: those names are the table of the plain, psy and first nr instantiations, tests/mb_instantiations.py.)
#include "k_mb.hip.h"

namespace x264gpu {
void launch_nr_any_slice_b_hex(const EncK &k, int streams, hipStream_t st)
{
    if (!k.rd || k.subme < 7) mb_launch_nr_any<2, 1, 0, true>(k, streams, st);
    else if (!k.cabac) mb_launch_nr_any<2, 1, 1, true>(k, streams, st);
    else mb_launch_nr_any<2, 1, 2, true>(k, streams, st);
}
}  // namespace x264gpu

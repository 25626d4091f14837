// nr_any_slice_t_esa.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction in CABAC trellis sessions under --me esa (x264gpu_encoder_set_nr_any; me hex
// / umh have these in mb_slice_nr_*.hip): P slices with trellis 1 (RD 3) and trellis 2 (RD 4), B slices analysed without RD (RD 7), with RD and trellis 1 / 2.
// (Not mb_slice_*.hip, not mb_launch: those names are the table of the plain, psy and first nr instantiations, tests/mb_instantiations.py.)
#include "k_mb.hip.h"

namespace x264gpu {
void launch_nr_any_slice_t_esa(const EncK &k, int streams, bool bslice, hipStream_t st)
{
    if (!bslice) {
        if (k.trellis & 64) mb_launch_nr_any<2, 3, 4>(k, streams, st);
        else mb_launch_nr_any<2, 3, 3>(k, streams, st);
    } else if (k.subme < 7) mb_launch_nr_any<2, 3, 7, true>(k, streams, st);
    else if (k.trellis & 64) mb_launch_nr_any<2, 3, 4, true>(k, streams, st);
    else mb_launch_nr_any<2, 3, 3, true>(k, streams, st);
}
}  // namespace x264gpu

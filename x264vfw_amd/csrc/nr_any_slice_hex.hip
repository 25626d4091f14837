// nr_any_slice_hex.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction in the toolsets x264gpu_encoder_set_nr_any adds (the NR siblings of the
// plain instantiations: the same decisions, every inter residual denoised before it is quantised), P slices under --me hex: without RD (both sub-pel margins), RD
// with CAVLC bit counts, RD with CABAC sizes; a translation unit of its own so that the instantiations build in parallel.
// (Not mb_slice_*.hip, not mb_launch: those names are the table of the plain, psy and first nr instantiations, tests/mb_instantiations.py.)
#include "k_mb.hip.h"

namespace x264gpu {
void launch_nr_any_slice_hex(const EncK &k, int streams, bool big_margin, hipStream_t st)
{
    if (k.rd && k.cabac) mb_launch_nr_any<2, 1, 2>(k, streams, st);
    else if (k.rd) mb_launch_nr_any<2, 1, 1>(k, streams, st);
    else if (big_margin) mb_launch_nr_any<5, 1, 0>(k, streams, st);
    else mb_launch_nr_any<2, 1, 0>(k, streams, st);
}
}  // namespace x264gpu

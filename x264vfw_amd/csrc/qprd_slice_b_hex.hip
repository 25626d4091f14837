// qprd_slice_b_hex.hip — the macroblock-loop kernel (k_mb.hip.h) with x264's QP-RD (--subme 10, cfg.qp_rd: the QPRD instantiations, which after a macroblock's
// decision walk the neighbouring quantisers with candidate passes, qprd.hip.h), B slices under --me hex; a translation unit of its own so that the instantiations build in
// parallel.  QP-RD sessions are CABAC sessions with RD refinement and --trellis 2 under --me hex / umh (x264gpu_encoder_create checks): RD 6 only.
// (Not mb_slice_*.hip, not mb_launch: those names are the table of the plain, psy and nr instantiations, tests/mb_instantiations.py.)
#include "k_mb.hip.h"

namespace x264gpu {
void launch_qprd_slice_b_hex(const EncK &k, int streams, hipStream_t st) { mb_launch_qprd<5, 1, true, 6, true>(k, streams, st); }
}  // namespace x264gpu

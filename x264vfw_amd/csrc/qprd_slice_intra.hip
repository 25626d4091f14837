// qprd_slice_intra.hip — the macroblock-loop kernel (k_mb.hip.h) with x264's QP-RD (--subme 10, cfg.qp_rd: the QPRD instantiations, which after a macroblock's
// decision walk the neighbouring quantisers with candidate passes, qprd.hip.h), I slices, and the choice among the QP-RD units; a translation unit of its own so that the instantiations build in
// parallel.  QP-RD sessions are CABAC sessions with RD refinement and --trellis 2 under --me hex / umh (x264gpu_encoder_create checks): RD 6 only.
// (Not mb_slice_*.hip, not mb_launch: those names are the table of the plain, psy and nr instantiations, tests/mb_instantiations.py.)
#include "k_mb.hip.h"

namespace x264gpu {
void launch_qprd_slice_hex(const EncK &k, int streams, hipStream_t st);
void launch_qprd_slice_umh(const EncK &k, int streams, hipStream_t st);
void launch_qprd_slice_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_qprd_slice_b_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_qprd(const EncK &k, int streams, int slice_type, hipStream_t st)
{
    const bool umh = k.me_method == 2;
    if (slice_type == X264GPU_SLICE_I) mb_launch_qprd<2, 1, false, 6>(k, streams, st);
    else if (slice_type == X264GPU_SLICE_B) (umh ? launch_qprd_slice_b_umh : launch_qprd_slice_b_hex)(k, streams, st);
    else (umh ? launch_qprd_slice_umh : launch_qprd_slice_hex)(k, streams, st);
}
}  // namespace x264gpu

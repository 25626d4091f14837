// mb_slice_psy_intra.hip — the macroblock-loop kernel (k_mb.hip.h) with psy-trellis (cfg.psy_trellis_q8 != 0: the PSY instantiations, which hold the
// source transform of every macroblock and run the psy variant of the trellis search at the luma sites), I slices (RD 3 .. 6), and the choice among all psy units; a translation unit of its own so
// that the instantiations build in parallel.  The selection mirrors the plain units'.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_psy_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_ref_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_ref_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_ref_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_b_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_psy_ref_b_umh(const EncK &k, int streams, hipStream_t st);
// psy sessions are RD sessions with CABAC and the trellis quantiser under --me hex / umh (x264gpu_encoder_create checks)
void launch_mb_slice_psy(const EncK &k, int streams, int slice_type, hipStream_t st)
{
    const bool umh = k.me_method == 2;
    if (slice_type == X264GPU_SLICE_I) {
        if ((k.rd >> 1) & 63) {          // RD refinement (subme 8)
            if (k.trellis & 64) mb_launch<2, 1, false, 6, false, true>(k, streams, st);
            else mb_launch<2, 1, false, 5, false, true>(k, streams, st);
        } else if (k.trellis & 64) mb_launch<2, 1, false, 4, false, true>(k, streams, st);
        else mb_launch<2, 1, false, 3, false, true>(k, streams, st);
    } else if (slice_type == X264GPU_SLICE_B) {
        if (k.subme >= 9 || (k.rd & 64)) (umh ? launch_mb_slice_psy_ref_b_umh : launch_mb_slice_psy_ref_b_hex)(k, streams, st);
        else (umh ? launch_mb_slice_psy_b_umh : launch_mb_slice_psy_b_hex)(k, streams, st);
    } else {
        if (((k.rd >> 1) & 63) || k.subme >= 8) (umh ? launch_mb_slice_psy_ref_umh : launch_mb_slice_psy_ref_hex)(k, streams, st);
        else (umh ? launch_mb_slice_psy_umh : launch_mb_slice_psy_hex)(k, streams, st);
    }
}
}  // namespace x264gpu

// mb_slice_nr_hex.hip — the macroblock-loop kernel (k_mb.hip.h) with noise reduction (x264gpu_encoder_set_nr: the NR instantiations, which denoise every inter
// residual they transform with the stream's offsets and gather the statistics of the final encodes), P slices under --me hex, trellis 1 (RD 3) and trellis 2 (RD 4); a translation unit of its own so
// that the instantiations build in parallel.  The selection mirrors the psy units'.
#include "k_mb.hip.h"

namespace x264gpu {
void launch_mb_slice_nr_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_b_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_b_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_hex(const EncK &k, int streams, hipStream_t st)
{
    if (k.trellis & 64) mb_launch<2, 1, true, 4, false, false, true>(k, streams, st);
    else mb_launch<2, 1, true, 3, false, false, true>(k, streams, st);
}
// nr sessions are RD sessions with CABAC and the trellis quantiser under --me hex / umh (x264gpu_encoder_set_nr checks); I slices run the plain kernels
void launch_mb_slice_nr(const EncK &k, int streams, int slice_type, hipStream_t st)
{
    const bool umh = k.me_method == 2;
    if (slice_type == X264GPU_SLICE_B) {
        if (k.subme >= 9 || (k.rd & 64)) (umh ? launch_mb_slice_nr_ref_b_umh : launch_mb_slice_nr_ref_b_hex)(k, streams, st);
        else (umh ? launch_mb_slice_nr_b_umh : launch_mb_slice_nr_b_hex)(k, streams, st);
    } else {
        if (((k.rd >> 1) & 63) || k.subme >= 8) (umh ? launch_mb_slice_nr_ref_umh : launch_mb_slice_nr_ref_hex)(k, streams, st);
        else (umh ? launch_mb_slice_nr_umh : launch_mb_slice_nr_hex)(k, streams, st);
    }
}
}  // namespace x264gpu

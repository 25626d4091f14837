// nr_any_slice.hip — which denoising instantiation of the macroblock loop a session of x264gpu_encoder_set_nr_any launches when it lies outside the toolset of
// x264gpu_encoder_set_nr (encoder.hip tells the two apart): the selection mirrors the plain launchers' (mb_slice_<me>.hip, mb_slice_b*.hip), kernel for kernel —
// the NR sibling of what the session would run without --nr.  Host code only; the kernels are in nr_any_slice_<me>.hip (P slices: no RD, CAVLC bit counts, CABAC
// sizes), nr_any_slice_b_<me>.hip (B slices: the same) and nr_any_slice_t_dia / _esa.hip (the trellis levels me hex / umh have in mb_slice_nr_*.hip).
#include "k_mb.hip.h"

namespace x264gpu {
void launch_nr_any_slice_dia(const EncK &k, int streams, bool big_margin, hipStream_t st);
void launch_nr_any_slice_hex(const EncK &k, int streams, bool big_margin, hipStream_t st);
void launch_nr_any_slice_umh(const EncK &k, int streams, bool big_margin, hipStream_t st);
void launch_nr_any_slice_esa(const EncK &k, int streams, bool big_margin, hipStream_t st);
void launch_nr_any_slice_b_dia(const EncK &k, int streams, hipStream_t st);
void launch_nr_any_slice_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_nr_any_slice_b_umh(const EncK &k, int streams, hipStream_t st);
void launch_nr_any_slice_b_esa(const EncK &k, int streams, hipStream_t st);
void launch_nr_any_slice_t_dia(const EncK &k, int streams, bool bslice, hipStream_t st);
void launch_nr_any_slice_t_esa(const EncK &k, int streams, bool bslice, hipStream_t st);
void launch_mb_slice_nr(const EncK &k, int streams, int slice_type, hipStream_t st);                 // mb_slice_nr_hex.hip
void launch_mb_slice_nr_ref_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_umh(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_b_hex(const EncK &k, int streams, hipStream_t st);
void launch_mb_slice_nr_ref_b_umh(const EncK &k, int streams, hipStream_t st);

void launch_nr_any_slice(const EncK &k, int streams, int slice_type, hipStream_t st)
{
    const bool bslice = slice_type == X264GPU_SLICE_B, hexumh = k.me_method == 1 || k.me_method == 2, umh = k.me_method == 2, cabac_rd = k.rd && k.cabac;
    // CABAC trellis sessions: me hex / umh own these kernels since x264gpu_encoder_set_nr (encoder.hip sends them there itself; kept for a caller that does not)
    if (cabac_rd && k.trellis && hexumh) { launch_mb_slice_nr(k, streams, slice_type, st); return; }
    if (bslice) {
        const bool rd_b = k.rd && k.subme >= 7;          // (below --subme 7 B slices are analysed without RD)
        // RD refinement without the trellis quantiser (--subme 9 --trellis 0): RD 5, which the first nr units hold
        if (rd_b && k.cabac && hexumh && (k.subme >= 9 || (k.rd & 64))) { (umh ? launch_mb_slice_nr_ref_b_umh : launch_mb_slice_nr_ref_b_hex)(k, streams, st); return; }
        if (cabac_rd && k.trellis) { (k.me_method == 0 ? launch_nr_any_slice_t_dia : launch_nr_any_slice_t_esa)(k, streams, true, st); return; }
        (k.me_method == 0 ? launch_nr_any_slice_b_dia : k.me_method == 2 ? launch_nr_any_slice_b_umh : k.me_method == 3 ? launch_nr_any_slice_b_esa : launch_nr_any_slice_b_hex)(k, streams, st);
        return;
    }
    if (cabac_rd && hexumh && (((k.rd >> 1) & 63) || k.subme >= 8)) { (umh ? launch_mb_slice_nr_ref_umh : launch_mb_slice_nr_ref_hex)(k, streams, st); return; }      // (--subme 8 / 9 --trellis 0: RD 5)
    if (cabac_rd && k.trellis) { (k.me_method == 0 ? launch_nr_any_slice_t_dia : launch_nr_any_slice_t_esa)(k, streams, false, st); return; }
    (k.me_method == 0 ? launch_nr_any_slice_dia : k.me_method == 2 ? launch_nr_any_slice_umh : k.me_method == 3 ? launch_nr_any_slice_esa : launch_nr_any_slice_hex)(k, streams, k.subme >= 8, st);
}
}  // namespace x264gpu

// siderows.hpp — a round's side inputs for a device encoder with several streams: every stream's quantiser-offset row and its two rows of low-resolution vectors
// (what a session on its own hands x264gpu_encoder_set_mb_qp_offsets / _set_lowres_mvs / _set_lowres_mvs1) lie anywhere in device memory and become the encoder's
// [streams][mb_count] arrays.  The cross-session batcher (host/batch.cpp: a row per member) and the GOP slots with quantisers planned ahead (host/gopslots.cpp: a
// row per slot, out of the plan store) call this one implementation.
#pragma once
#include "host.hpp"

namespace x264host {

// the row that stands in for a stream without vectors among streams with them: nmb vectors, the first entry 0x7fff (x264gpu_encoder_set_lowres_mvs: "absent" is
// a row that says so, not a row of zero vectors).  On the current device; nullptr: failed (the device's last error set)
int16_t *side_rows_absent(size_t nmb);

// tab: [3][N] row pointers (array a's row of stream s at a * N + s; nullptr: a row of zeros), any[a]: array a is gathered at all.  Every gathered array lands in
// d_dst[a] as [N][row] bytes on stream st: one x264gpu_gather_rows launch an array, behind the table's upload into d_tab ([3][N] pointers on the device) on
// tab_stream — or, with a device library without the gather entry (an older build; the tests' CPU stand-in), row by row.  false: the device's last error set
bool side_rows_gather(const void *const *tab, const bool any[3], const void **d_tab, uint8_t *const d_dst[3], size_t N, size_t row, void *st, void *tab_stream);

}  // namespace x264host

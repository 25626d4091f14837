// noisereduction.hpp — --nr of the host encoder (x264 analyse.i_noise_reduction; [x264-upstream] encoder/encoder.c x264_noise_reduction_update): which sessions
// run it, and the one state a session keeps on the device — running sums, counts and the offsets the next picture is denoised with (x264gpu_encoder_set_nr,
// x264gpu_nr_update).  The state moves on once per ACCEPTED picture, in coding order: a picture coded again (the VBV guard) sees the offsets of its first issue.
#pragma once
#include "host.hpp"

namespace x264host {

// the device entries through their weak bindings (EINVAL when the device library lacks them): what the batcher calls for a group's streams
// (any: through x264gpu_encoder_set_nr_any, the entry that admits every inter toolset — sessions settled under X264GPU_NR_ANY=1)
int nr_set(x264gpu_encoder *gpu, const x264gpu_nr_offsets *d_off, x264gpu_nr_sums *d_pic, bool any);
int nr_update_queue(x264gpu_nr_offsets *d_off, x264gpu_nr_sums *d_state, const x264gpu_nr_sums *d_pic, int streams, int strength, void *stream);

struct NoiseReduction {
    int strength = 0;                    // what runs (0: the session does nothing of this)
    x264gpu_nr_offsets *d_off = nullptr; x264gpu_nr_sums *d_state = nullptr, *d_pic = nullptr;

    // the rules that hang on the toolset alone (before psy-trellis is settled: nr wins over it): clips the strength to 0 .. 65536; one WARNING that names what is
    // missing, and nr 0, when the device library has no nr entries or the session is not a CABAC trellis session at subme >= 6 under me hex / umh
    // want_any (X264GPU_NR_ANY=1): with a device library that has x264gpu_encoder_set_nr_any the entries are the whole rule — any entropy coder, subme, trellis and
    // search method; returns whether the session was admitted that way (it then runs on the DPB model and opens through that entry).  Without the entry: the rules above
    static bool check_toolset(x264_param_t &p, bool want_any);
    // ... on the session's mode: needs the DPB model (a batch group runs on it) and one GOP.  Runs before psy-trellis gives way: what is refused here leaves it alone
    static void check_modes(x264_param_t &p, bool dpbmode);
    // zeroed state and offsets on the device, the encoder told to denoise with them; false: a device call failed (the rules above are the device's: it takes what they pass)
    bool open(x264_param_t &p, x264gpu_encoder *gpu, bool any);
    // the picture the encoder coded last is accepted: its statistics join the state, the next picture's offsets follow (queued on `stream`)
    int accepted(void *stream) const;
    int offsets(uint16_t out[3][64]) const;
    void close();
};

}  // namespace x264host

// noisereduction.cpp — --nr: which sessions run it and the session's state on the device (host/noisereduction.hpp).
#include "noisereduction.hpp"
#include "../../include/x264gpu_host.h"
#include <string.h>

// The device entries are resolved weakly: a device library without them (an older build; the tests' CPU stand-in) still loads, and the session runs nr 0.
#pragma weak x264gpu_encoder_set_nr
#pragma weak x264gpu_encoder_set_nr_any
#pragma weak x264gpu_nr_update
#pragma weak x264gpu_denoise_blocks

namespace x264host {

int nr_set(x264gpu_encoder *gpu, const x264gpu_nr_offsets *d_off, x264gpu_nr_sums *d_pic, bool any)
{
    if (any) return x264gpu_encoder_set_nr_any ? x264gpu_encoder_set_nr_any(gpu, d_off, d_pic) : X264GPU_EINVAL;
    return x264gpu_encoder_set_nr ? x264gpu_encoder_set_nr(gpu, d_off, d_pic) : X264GPU_EINVAL;
}

int nr_update_queue(x264gpu_nr_offsets *d_off, x264gpu_nr_sums *d_state, const x264gpu_nr_sums *d_pic, int streams, int strength, void *stream)
{
    return x264gpu_nr_update ? x264gpu_nr_update(d_off, d_state, d_pic, streams, strength, stream) : X264GPU_EINVAL;
}

bool NoiseReduction::check_toolset(x264_param_t &p, bool want_any)
{
    int &nr = p.analyse.i_noise_reduction;
    nr = clampi(nr, 0, 65536);
    if (!nr) return false;
    // the extended toolset (X264GPU_NR_ANY=1): the device entries are all it takes; a device library without x264gpu_encoder_set_nr_any: the rules below
    if (want_any && x264gpu_encoder_set_nr_any && x264gpu_encoder_set_nr && x264gpu_nr_update && x264gpu_denoise_blocks) return true;
    const char *missing = !x264gpu_encoder_set_nr || !x264gpu_nr_update || !x264gpu_denoise_blocks ? "a device library with the nr entries" :
                          !p.b_cabac ? "CABAC" : p.analyse.i_subpel_refine < 6 ? "subme >= 6" : p.analyse.i_trellis < 1 ? "trellis >= 1" :
                          p.analyse.i_me_method != X264_ME_HEX && p.analyse.i_me_method != X264_ME_UMH ? "me hex / umh" : nullptr;
    if (missing) { xlog(&p, X264_LOG_WARNING, "nr (noise reduction) needs %s in the MI355X path (the denoising macroblock loop is built for CABAC trellis sessions under me hex / umh): nr 0\n", missing); nr = 0; }
    return false;
}

void NoiseReduction::check_modes(x264_param_t &p, bool dpbmode)
{
    int &nr = p.analyse.i_noise_reduction;
    if (!nr) return;
    const char *missing = p.i_threads > 1 ? "threads 1 (GOP slots are coded in lock-step: the state of one GOP cannot follow the one before)" :
                          !dpbmode ? "B-frames, weightp 2 or VBV (the DPB-model path, one picture at a time)" : nullptr;
    if (missing) { xlog(&p, X264_LOG_WARNING, "nr (noise reduction) needs %s in the MI355X path: nr 0\n", missing); nr = 0; }
}

bool NoiseReduction::open(x264_param_t &p, x264gpu_encoder *gpu, bool any)
{
    strength = p.analyse.i_noise_reduction;
    if (!strength) return true;
    if (x264gpu_malloc((void **)&d_off, sizeof(*d_off)) != X264GPU_OK || x264gpu_malloc((void **)&d_state, sizeof(*d_state)) != X264GPU_OK ||
        x264gpu_malloc((void **)&d_pic, sizeof(*d_pic)) != X264GPU_OK) return false;
    if (x264gpu_memset(d_off, 0, sizeof(*d_off), nullptr) != X264GPU_OK || x264gpu_memset(d_state, 0, sizeof(*d_state), nullptr) != X264GPU_OK ||
        x264gpu_memset(d_pic, 0, sizeof(*d_pic), nullptr) != X264GPU_OK) return false;
    return nr_set(gpu, d_off, d_pic, any) == X264GPU_OK;
}

int NoiseReduction::accepted(void *stream) const
{
    if (!strength) return X264GPU_OK;
    return x264gpu_nr_update(d_off, d_state, d_pic, 1, strength, stream);
}

int NoiseReduction::offsets(uint16_t out[3][64]) const
{
    if (!strength) { memset(out, 0, 3 * 64 * sizeof(uint16_t)); return -1; }
    if (x264gpu_stream_sync(nullptr) != X264GPU_OK || x264gpu_memcpy_d2h(out, d_off, sizeof(*d_off), nullptr) != X264GPU_OK || x264gpu_stream_sync(nullptr) != X264GPU_OK) return -1;
    return 0;
}

void NoiseReduction::close()
{
    if (d_off) x264gpu_free(d_off);
    if (d_state) x264gpu_free(d_state);
    if (d_pic) x264gpu_free(d_pic);
    d_off = nullptr; d_state = d_pic = nullptr; strength = 0;
}

}  // namespace x264host

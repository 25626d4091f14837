// quality.hpp — --psnr / --ssim of the host encoder (x264 analyse.b_psnr / b_ssim; [x264-upstream] encoder/encoder.c encoder_frame_end and the closing
// statistics of x264_encoder_close, restated): what a session keeps of the device's per-picture statistics (x264gpu_encoder_quality) and the x264-style log lines.
#pragma once
#include "host.hpp"
#include <string>

namespace x264host {

// x264gpu_encoder_quality through its weak binding (EINVAL when the device library lacks it)
int quality_queue(x264gpu_encoder *gpu, int flags, x264gpu_quality *d_out, void *stream);

struct Quality {
    int flags = 0;                       // X264GPU_QUALITY_PSNR | _SSIM; 0: the session does nothing of this (no allocation, no device call, no log line)
    int w = 0, h = 0;
    // the picture handed back last (x264host_last_quality)
    bool have_last = false;
    double last_psnr[4] = { 0, 0, 0, 0 }, last_ssim = 0;
    uint64_t last_ssd[3] = { 0, 0, 0 };
    // per slice type (0 I, 1 P, 2 B), every picture weighted alike (x264 weights by duration under vfr): h->stat.i_frame_count / f_frame_qp / i_frame_size /
    // f_psnr_mean_y, _u, _v / f_psnr_average / f_ssd_global / f_ssim_mean_y
    struct Acc { long n = 0; double qp = 0, bytes = 0, psnr[4] = { 0, 0, 0, 0 }, ssd = 0, ssim = 0; } acc[3];
    long frames = 0;

    // flags from the parameters; 0 with one WARNING when the device library has no quality entry, with one INFO line for GOP-slot sessions
    void open(const x264_param_t &p, bool gop_slots);
    // queues the statistic of the picture `gpu` coded last on `stream` into d_out[streams]
    int queue(x264gpu_encoder *gpu, x264gpu_quality *d_out, void *stream) const { return quality_queue(gpu, flags, d_out, stream); }
    // a picture leaves: its figures, the sums, the DEBUG line.  type: 0 I, 1 P, 2 B
    void frame_end(const x264_param_t &p, const x264gpu_quality &q, int type, double qp, int poc, size_t bytes);
    // the closing lines, one '\n' behind each
    std::string summary(const x264_param_t &p) const;
    void log_summary(const x264_param_t &p) const;
};
double mean_mb_qp(const x264gpu_mb *mbs, size_t n);          // x264 fdec->f_qp_avg_aq

}  // namespace x264host

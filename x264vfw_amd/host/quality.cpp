// quality.cpp — --psnr / --ssim: per-picture and per-session figures from the device's statistics, x264's log lines (host/quality.hpp).
#include "quality.hpp"
#include "../../include/x264gpu_host.h"
#include <math.h>
#include <stdarg.h>
#include <stdio.h>

// The device entry is resolved weakly: a device library without it (an older build; the tests' CPU stand-in) still loads, and the session runs as without the flags.
#pragma weak x264gpu_encoder_quality

using namespace x264host;

extern "C" {

// x264_psnr: sqe = the sum of squared differences over `n` samples
double x264host_psnr(double ssd, double n)
{
    const double mse = ssd / (255.0 * 255.0 * n);
    if (mse <= 0.0000000001) return 100;          // max 100 dB
    return -10.0 * log10(mse);
}

// x264_ssim: the mean window value in dB
double x264host_ssim_db(double ssim)
{
    const double inv = 1.0 - ssim;
    if (inv <= 0.0000000001) return 100;
    return -10.0 * log10(inv);
}

}  // extern "C"

namespace x264host {

static void appendf(std::string &s, const char *fmt, ...)
{
    char buf[512];
    va_list ap;
    va_start(ap, fmt);
    vsnprintf(buf, sizeof(buf), fmt, ap);
    va_end(ap);
    s += buf;
}

double mean_mb_qp(const x264gpu_mb *mbs, size_t n)
{
    double s = 0;
    for (size_t i = 0; i < n; i++) s += mbs[i].qp;
    return n ? s / (double)n : 0;
}

void Quality::open(const x264_param_t &p, bool gop_slots)
{
    w = p.i_width; h = p.i_height;
    flags = (p.analyse.b_psnr ? X264GPU_QUALITY_PSNR : 0) | (p.analyse.b_ssim ? X264GPU_QUALITY_SSIM : 0);
    if (!flags) return;
    if (!x264gpu_encoder_quality) { xlog(&p, X264_LOG_WARNING, "psnr / ssim: the device library has no quality entry\n"); flags = 0; return; }
    if (gop_slots) { xlog(&p, X264_LOG_INFO, "psnr / ssim switched off in GOP-slot sessions (--threads %d: pictures of several GOPs are coded per call)\n", p.i_threads); flags = 0; }
}

int quality_queue(x264gpu_encoder *gpu, int flags, x264gpu_quality *d_out, void *stream)
{
    if (!flags || !x264gpu_encoder_quality) return X264GPU_EINVAL;
    return x264gpu_encoder_quality(gpu, flags, d_out, stream);
}

void Quality::frame_end(const x264_param_t &p, const x264gpu_quality &q, int type, double qp, int poc, size_t bytes)
{
    if (!flags) return;
    const double ny = (double)w * h, nc = ny / 4;
    Acc &a = acc[type];
    a.n++; a.qp += qp; a.bytes += (double)bytes;
    std::string line;
    appendf(line, "frame=%4ld QP=%.2f Slice:%c Poc:%-3d size=%d bytes", frames, qp, "IPB"[type], poc, (int)bytes);
    for (int i = 0; i < 4; i++) last_psnr[i] = 0;
    last_ssim = 0;
    for (int i = 0; i < 3; i++) last_ssd[i] = q.ssd[i];
    if (flags & X264GPU_QUALITY_PSNR) {
        const double all = (double)q.ssd[0] + (double)q.ssd[1] + (double)q.ssd[2];
        last_psnr[0] = x264host_psnr((double)q.ssd[0], ny); last_psnr[1] = x264host_psnr((double)q.ssd[1], nc); last_psnr[2] = x264host_psnr((double)q.ssd[2], nc);
        last_psnr[3] = x264host_psnr(all, 3 * ny / 2);
        for (int i = 0; i < 4; i++) a.psnr[i] += last_psnr[i];
        a.ssd += all;
        appendf(line, " PSNR Y:%5.2f U:%5.2f V:%5.2f", last_psnr[0], last_psnr[1], last_psnr[2]);
    }
    if (flags & X264GPU_QUALITY_SSIM) {
        last_ssim = q.ssim_cnt ? q.ssim_sum / (double)q.ssim_cnt : 0;
        a.ssim += last_ssim;
        appendf(line, " SSIM Y:%.5f", last_ssim);
    }
    have_last = true;
    frames++;
    xlog(&p, X264_LOG_DEBUG, "%s\n", line.c_str());
}

std::string Quality::summary(const x264_param_t &p) const
{
    std::string s;
    if (!flags || !frames) return s;
    const double pixels = 3.0 * w * h / 2;
    long n = 0; double bytes = 0, ps[4] = { 0, 0, 0, 0 }, ssd = 0, ssim = 0;
    for (int t = 0; t < 3; t++) {
        const Acc &a = acc[t];
        n += a.n; bytes += a.bytes; ssd += a.ssd; ssim += a.ssim;
        for (int i = 0; i < 4; i++) ps[i] += a.psnr[i];
        if (!a.n) continue;
        appendf(s, "frame %c:%-5ld Avg QP:%5.2f  size:%6.0f", "IPB"[t], a.n, a.qp / a.n, a.bytes / a.n);
        if (flags & X264GPU_QUALITY_PSNR)
            appendf(s, "  PSNR Mean Y:%5.2f U:%5.2f V:%5.2f Avg:%5.2f Global:%5.2f", a.psnr[0] / a.n, a.psnr[1] / a.n, a.psnr[2] / a.n, a.psnr[3] / a.n, x264host_psnr(a.ssd, (double)a.n * pixels));
        s += "\n";
    }
    if (flags & X264GPU_QUALITY_SSIM) appendf(s, "SSIM Mean Y:%.7f (%6.3fdb)\n", ssim / n, x264host_ssim_db(ssim / n));
    if (flags & X264GPU_QUALITY_PSNR) {
        const double fps = p.i_fps_num && p.i_fps_den ? (double)p.i_fps_num / p.i_fps_den : 25.0;
        appendf(s, "PSNR Mean Y:%6.3f U:%6.3f V:%6.3f Avg:%6.3f Global:%6.3f kb/s:%.2f\n", ps[0] / n, ps[1] / n, ps[2] / n, ps[3] / n, x264host_psnr(ssd, (double)n * pixels),
                bytes / n / 125.0 * fps);
    }
    return s;
}

void Quality::log_summary(const x264_param_t &p) const
{
    const std::string s = summary(p);
    for (size_t at = 0; at < s.size();) {
        const size_t nl = s.find('\n', at);
        xlog(&p, X264_LOG_INFO, "%s\n", s.substr(at, nl - at).c_str());
        at = nl + 1;
    }
}

}  // namespace x264host

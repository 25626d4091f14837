"""Sessions through x264_encoder_* with --psnr / --ssim for the quality tests: every picture's x264host_last_quality and reconstruction as it leaves, the
closing summary (x264host_quality_summary) and the text of what the session logged through pf_log."""
import ctypes as C

import numpy as np

import host_lib as HL

H = HL.H
_libc = C.CDLL(None)
_libc.vsnprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p]
LOG_CB = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p)


def make_logger(sink):
    """a pf_log that formats the message (x86-64: a va_list argument is a pointer) and appends (level, text) to sink; keep the returned object alive"""
    def cb(priv, lvl, fmt, va):
        buf = C.create_string_buffer(2048)
        _libc.vsnprintf(buf, 2048, fmt, va)
        sink.append((lvl, buf.value.decode(errors="replace")))
    return LOG_CB(cb)


def run_session(w, h, frames, opts, quality=True, log_level=2, preset=b"medium", want_recon=True):
    """-> dict(stream, pics = [dict(pts, type, rc, psnr[4], ssim, ssd[3], recon)], summary, summary_rc, log = [(level, text)])"""
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset, None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    opts = dict(opts)
    if quality:
        opts.update({"psnr": None, "ssim": None} if quality is True else quality)
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, log_level
    p.b_vfr_input = 0
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_, "x264_encoder_open failed"
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, n = C.POINTER(HL.Nal)(), C.c_int()
    res = dict(stream=b"", pics=[], log=log)

    def take(size):
        assert size >= 0, "x264_encoder_encode failed"
        if not size:
            return
        res["stream"] += C.string_at(nal[0].p_payload, size)
        ps, ss, sd = (C.c_double * 4)(), C.c_double(), (C.c_uint64 * 3)()
        rc = H.x264host_last_quality(h_, ps, C.byref(ss), sd)
        rec = None
        if want_recon:
            rec = np.zeros(w * h * 3 // 2, np.uint8)
            assert H.x264host_get_recon(h_, rec.ctypes.data) == 0
        res["pics"].append(dict(pts=int(out.i_pts), type=int(out.i_type), size=size, rc=rc, psnr=list(ps), ssim=ss.value, ssd=[int(x) for x in sd], recon=rec))
    for i, f in enumerate(frames):
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(n), C.byref(pic), C.byref(out)))
    while H.x264_encoder_delayed_frames(h_):
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(n), None, C.byref(out))
        assert size > 0
        take(size)
    buf = C.create_string_buffer(4096)
    res["summary_rc"] = H.x264host_quality_summary(h_, buf, 4096)
    res["summary"] = buf.value.decode()
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return res

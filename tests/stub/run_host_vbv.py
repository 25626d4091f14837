#!/usr/bin/env python3
"""A VBV session (--vbv-maxrate / --vbv-bufsize / --nal-hrd) through x264_encoder_encode(): per returned picture its type, timestamps and size, the lookahead
decision (x264host_last_decision / _last_qpm) and the rate control's view of it (x264host_last_vbv); the effective parameters, the log, the stream and the
reconstruction of the last coded picture.  session() runs in the caller's process on whatever host library it has loaded (the device tests); as a program it runs
over the STUB-backed host library and prints one JSON line.  Usage: run_host_vbv.py OUT W H FRAMES SEED key=value ...  (OUT: the stream; OUT.recon: the
reconstruction)"""
import ctypes as C
import json
import os
import sys


def session(HL, frames, w, h, opts, fps=(25, 1), preset=b"medium"):
    """opts: {option: value or None}.  -> (info dict, stream bytes, reconstruction of the last coded picture as bytes)"""
    H = HL.H
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset, None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = fps
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p)(lambda priv, lvl, fmt, va: log.append([lvl, fmt.decode(errors="replace").strip()]))
    p.pf_log = C.cast(cb, C.c_void_p).value
    p.i_log_level = 3
    p.b_vfr_input = 0                                                  # the driver forces constant frame rate (codec.c:1476-1480)
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    planes = [(w * h, 0), (w * h // 4, w * h), (w * h // 4, w * h * 5 // 4)]
    stream, recs, vbv, decisions, nal_types = b"", [], [], [], []

    def take(size):
        nonlocal stream
        if size <= 0:
            return
        stream += C.string_at(nal[0].p_payload, size)
        recs.append((out.i_type, out.i_pts, out.i_dts, out.b_keyframe, size))
        nal_types.append([nal[i].i_type for i in range(nn.value)])
        qp, sc, costs = C.c_int(), C.c_int(), (C.c_int32 * 4)()
        assert H.x264host_last_decision(h_, C.byref(qp), C.byref(sc), costs) == 0
        decisions.append([qp.value, sc.value, list(costs), float(H.x264host_last_qpm(h_))])
        vbv.append(HL.last_vbv(h_))
    for i, f in enumerate(frames):
        for pl, (sz, off) in enumerate(planes):
            C.memmove(pic.img.plane[pl], f[off:off + sz].ctypes.data, sz)
        pic.i_pts = i
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out))
        assert size >= 0
        take(size)
    while H.x264_encoder_delayed_frames(h_):
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out))
        assert size > 0
        take(size)
    recon = (C.c_uint8 * (w * h * 3 // 2))()
    have_recon = H.x264host_get_recon(h_, recon) == 0          # (GOP slots keep no single "last picture")
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    info = {"recs": recs, "vbv": vbv, "decisions": decisions, "nal_types": nal_types, "log": log,
            "eff": {"vbv_maxrate": eff.rc.i_vbv_max_bitrate, "vbv_bufsize": eff.rc.i_vbv_buffer_size, "vbv_init": eff.rc.f_vbv_buffer_init, "nal_hrd": eff.i_nal_hrd,
                    "bitrate": eff.rc.i_bitrate, "rc_method": eff.rc.i_rc_method, "lookahead": eff.rc.i_lookahead, "mbtree": eff.rc.b_mb_tree, "bframes": eff.i_bframe,
                    "weightp": eff.analyse.i_weighted_pred, "threads": eff.i_threads, "qp_min": eff.rc.i_qp_min, "qp_max": eff.rc.i_qp_max, "ipratio": eff.rc.f_ip_factor,
                    "pbratio": eff.rc.f_pb_factor, "level": eff.i_level_idc, "keyint": eff.i_keyint_max, "crf": eff.rc.f_rf_constant, "qcomp": eff.rc.f_qcompress,
                    "aq_mode": eff.rc.i_aq_mode, "ratetol": eff.rc.f_rate_tolerance, "qpstep": eff.rc.i_qp_step, "fps": [eff.i_fps_num, eff.i_fps_den]}}
    return info, stream, bytes(recon) if have_recon else b""


def main():
    os.environ["X264_HOST_STUB"] = "1"
    here = os.path.dirname(os.path.abspath(__file__))
    sys.path.insert(0, os.path.dirname(here))
    sys.path.insert(0, os.path.dirname(os.path.dirname(here)))
    sys.path.insert(0, here)
    import host_lib as HL
    from run_host_b import make_frames
    out_path = sys.argv[1]
    w, h, n, seed = (int(x) for x in sys.argv[2:6])
    opts = {}
    for a in sys.argv[6:]:
        k, eq, v = a.partition("=")
        opts[k] = v if eq else None
    scene_len = int(opts.pop("scene_len", 0) or 0)
    info, stream, recon = session(HL, make_frames(w, h, n, seed, scene_len), w, h, opts)
    open(out_path, "wb").write(stream)
    open(out_path + ".recon", "wb").write(recon)
    print(json.dumps(info))


if __name__ == "__main__":
    main()

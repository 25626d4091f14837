#!/usr/bin/env python3
"""A session through x264_encoder_encode() of the STUB-backed host library for the tests of GOP slots with quantisers planned ahead (X264GPU_GOP_SLOTS_RC, taken
from the environment as a user sets it): prints one JSON line — the stream's and the metadata's hashes (as run_host.py), x264host_gop_slots_planned when the
input has ended, the effective parameters, the log's format strings, per output picture the quantiser of x264host_last_decision and a hash of
x264host_last_mb_qp_offsets (serial sessions: GOP slots keep no single "last picture") — and writes the stream to OUT.
Usage: run_host_slots_rc.py OUT W H FRAMES SEED key=value ...   (x264 options; fade=<per cent a picture>: run_host_b.py's fading clip)"""
import ctypes as C
import hashlib
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))


def make_frames(w, h, n, seed, fade=0):
    """run_host_b.py's clips: synthetic frames, optionally fading to black by `fade` per cent a picture"""
    import numpy as np
    from synth import synth_frames
    frames = synth_frames(w, h, n, seed=seed)
    for i, f in enumerate(frames if fade else []):
        a = max(0.0, 1.0 - i * fade / 100.0)
        g = f.astype(np.float32)
        g[:w * h] *= a
        g[w * h:] = 128 + (g[w * h:] - 128) * a
        frames[i] = np.clip(np.rint(g), 0, 255).astype(np.uint8)
    return frames


def session(HL, out_path, w, h, n, seed, opts, stub=True):
    """the session on the host library HL binds (the stand-in build, or — tests/test_gpu_gop_slots_rc.py, stub=False — the product on the device); -> the result line as a dict"""
    import numpy as np
    opts = dict(opts)
    fade = int(opts.pop("fade", 0) or 0)
    H = HL.H
    frames = make_frames(w, h, n, seed, fade)
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p)(lambda priv, lvl, fmt, va: log.append([lvl, fmt.decode(errors="replace").strip()]))
    p.pf_log = C.cast(cb, C.c_void_p).value
    p.i_log_level = 2
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    planes = [(w * h, 0), (w * h // 4, w * h), (w * h // 4, w * h * 5 // 4)]
    stream, meta, qps, offs = b"", [], [], []
    serial = eff.i_threads <= 1
    first_out = None

    def take(size):
        nonlocal stream
        if size > 0:
            stream += C.string_at(nal[0].p_payload, size)
            meta.append((int(out.i_type), int(out.b_keyframe), int(out.i_pts), int(out.i_dts), [[int(nal[k].i_type), int(nal[k].i_ref_idc)] for k in range(nn.value)]))
            if serial:
                qp, sc, costs = C.c_int(), C.c_int(), (C.c_int32 * 4)()
                assert H.x264host_last_decision(h_, C.byref(qp), C.byref(sc), costs) == 0
                qps.append(qp.value)
                buf = np.zeros(nmb, np.float32)
                got = H.x264host_last_mb_qp_offsets(h_, buf.ctypes.data, nmb)
                offs.append(hashlib.sha256(buf.tobytes()).hexdigest()[:16] if got > 0 else None)
    for i, f in enumerate(frames):
        for pl, (sz, off) in enumerate(planes):
            C.memmove(pic.img.plane[pl], f[off:off + sz].ctypes.data, sz)
        pic.i_pts = i
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out))
        assert size >= 0, log[-3:]
        if size > 0 and first_out is None:
            first_out = i + 1
        take(size)
    delayed_at_end = H.x264_encoder_delayed_frames(h_)
    while H.x264_encoder_delayed_frames(h_):
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out))
        assert size > 0, log[-3:]
        take(size)
    planned = int(H.x264host_gop_slots_planned(h_))
    recons = []          # GOP slots: the reconstruction of the picture every slot coded last (OUT + ".recon": one tight I420 picture a slot)
    for sl in range(eff.i_threads if not serial else 0):
        buf = np.zeros(w * h * 3 // 2, np.uint8)
        assert H.x264host_gop_slots_recon(h_, sl, buf.ctypes.data) == 0
        recons.append(buf)
    if recons and out_path:
        np.concatenate(recons).tofile(out_path + ".recon")
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    if out_path:
        open(out_path, "wb").write(stream)
    calls = []
    if stub:
        lib = C.CDLL(os.path.join(HERE, "_build", "libx264gpu.so"))
        lib.x264gpu_stub_encode_calls.restype = C.c_long
        calls = [lib.x264gpu_stub_encode_calls(d) for d in range(int(os.environ.get("X264GPU_STUB_DEVICES", "2")))]
    return dict({"sha": hashlib.sha256(stream).hexdigest(), "bytes": len(stream), "frames": len(meta), "calls": calls, "planned": planned,
                      "meta": hashlib.sha256(json.dumps(meta).encode()).hexdigest(), "types": [m[0] for m in meta], "pts": [m[2] for m in meta], "dts": [m[3] for m in meta],
                      "ref_idc": [m[4] for m in meta], "qps": qps, "offsets": offs, "log": log, "first_output_after": first_out, "delayed_at_end": delayed_at_end,
                      "bframes": eff.i_bframe, "mbtree": eff.rc.b_mb_tree, "lookahead": eff.rc.i_lookahead, "aq_mode": eff.rc.i_aq_mode, "badapt": eff.i_bframe_adaptive,
                      "direct": eff.analyse.i_direct_mv_pred, "threads": eff.i_threads, "weightp": eff.analyse.i_weighted_pred, "rc_method": eff.rc.i_rc_method}, stream=stream)


def main():
    os.environ["X264_HOST_STUB"] = "1"
    sys.path.insert(0, os.path.dirname(HERE))
    sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
    import host_lib as HL
    out_path = sys.argv[1]
    w, h, n, seed = (int(x) for x in sys.argv[2:6])
    opts = {}
    for a in sys.argv[6:]:
        k, _, v = a.partition("=")
        opts[k] = v if _ else None
    res = session(HL, out_path, w, h, n, seed, opts)
    res.pop("stream")
    print(json.dumps(res))


if __name__ == "__main__":
    main()

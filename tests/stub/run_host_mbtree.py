#!/usr/bin/env python3
"""One session of a 2-pass encode through x264_encoder_encode() for the macroblock-tree statistics tests: over the STUB-backed host library, or (device=1) over
the product's own libraries on the GPU.  Prints one JSON line: the pictures as they leave (type, pts, dts, keyframe, size), the effective parameters, the log
(level, format string, formatted text), the second pass' plan (plan=1), and the call that failed, if one did (the session is closed behind it).  hook=1 writes
OUT + ".offsets": per output picture one byte (1: x264host_last_mb_qp_offsets had offsets) and nmb float32.
Usage: run_host_mbtree.py OUT W H FRAMES SEED key=value ... [-- OUT W H FRAMES SEED key=value ...]   (X264GPU_MBTREE_STATS comes from the caller's environment;
further sessions behind "--" run one after the other in the same process, a JSON line each)"""
import ctypes as C
import json
import os
import sys

DEVICE = "device=1" in sys.argv
if DEVICE:
    for k in ("X264_HOST_STUB", "X264GPU_HOST_LIB", "X264GPU_LIB"):
        os.environ.pop(k, None)
else:
    os.environ["X264_HOST_STUB"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import numpy as np  # noqa: E402
import host_lib as HL  # noqa: E402
from synth import synth_frames  # noqa: E402


def session(argv):
    out_path = argv[0]
    w, h, n, seed = (int(x) for x in argv[1:5])
    opts = {}
    for a in argv[5:]:
        k, eq, v = a.partition("=")
        opts[k] = v if eq else None
    opts.pop("device", None)
    H = HL.H
    scene_len = int(opts.pop("scene_len", 0) or 0)
    preset = (opts.pop("preset", None) or "medium").encode()
    want_plan = int(opts.pop("plan", 0) or 0)
    want_hook = int(opts.pop("hook", 0) or 0)
    frames = synth_frames(w, h, n, seed=seed, **({"scene_len": scene_len} if scene_len else {}))
    nmb = ((w + 15) // 16) * ((h + 15) // 16)
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset, None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    libc = C.CDLL(None)
    libc.vsnprintf.argtypes = [C.c_char_p, C.c_size_t, C.c_char_p, C.c_void_p]

    def on_log(priv, lvl, fmt, va):
        buf = C.create_string_buffer(1024)
        libc.vsnprintf(buf, 1024, fmt, va)
        log.append([lvl, fmt.decode(errors="replace").strip(), buf.value.decode(errors="replace").strip()])
    cb = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p)(on_log)
    p.pf_log = C.cast(cb, C.c_void_p).value
    p.i_log_level = 2          # X264_LOG_INFO
    p.b_vfr_input = 0
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    if not h_:
        print(json.dumps({"opened": False, "log": log}))
        return
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    plan = None
    if want_plan:
        qs, eb = (C.c_double * n)(), (C.c_double * n)()
        cnt = H.x264host_pass2_plan(h_, qs, eb, n)
        plan = {"count": cnt, "new_qscale": list(qs)[:cnt], "expected_bits": list(eb)[:cnt]}
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    planes = [(w * h, 0), (w * h // 4, w * h), (w * h // 4, w * h * 5 // 4)]
    stream, recs, qpm, offsets, failed_at = b"", [], [], b"", None

    def take(size):
        nonlocal stream, offsets
        stream += C.string_at(nal[0].p_payload, size)
        recs.append((out.i_type, out.i_pts, out.i_dts, out.b_keyframe, size))
        qp, sc, costs = C.c_int(), C.c_int(), (C.c_int32 * 4)()
        H.x264host_last_decision(h_, C.byref(qp), C.byref(sc), costs)
        qpm.append([qp.value, float(H.x264host_last_qpm(h_))])
        if want_hook:
            buf = np.zeros(nmb, np.float32)
            got = H.x264host_last_mb_qp_offsets(h_, buf.ctypes.data, nmb)
            assert got in (0, nmb), got
            offsets += bytes([1 if got else 0]) + buf.tobytes()
    for i, f in enumerate(frames):
        for pl, (sz, off) in enumerate(planes):
            C.memmove(pic.img.plane[pl], f[off:off + sz].ctypes.data, sz)
        pic.i_pts, pic.i_type = i, 0
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out))
        if size < 0:
            failed_at = i
            break
        if size > 0:
            take(size)
    while failed_at is None and H.x264_encoder_delayed_frames(h_):
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out))
        if size <= 0:
            failed_at = n
            break
        take(size)
    H.x264_encoder_close(h_)
    open(out_path, "wb").write(stream)
    if want_hook:
        open(out_path + ".offsets", "wb").write(offsets)
    print(json.dumps({"opened": True, "recs": recs, "qpm": qpm, "failed_at": failed_at, "mbtree": eff.rc.b_mb_tree, "rc_lookahead": eff.rc.i_lookahead, "bframes": eff.i_bframe,
                      "stat_read": eff.rc.b_stat_read, "stat_write": eff.rc.b_stat_write, "aq_mode": eff.rc.i_aq_mode, "aq_strength": eff.rc.f_aq_strength,
                      "log": log, "plan": plan}))


def main():
    argv = sys.argv[1:]
    while argv:
        cut = argv.index("--") if "--" in argv else len(argv)
        session(argv[:cut])
        argv = argv[cut + 1:]


if __name__ == "__main__":
    main()

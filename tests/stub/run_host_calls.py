#!/usr/bin/env python3
"""A session through x264_encoder_encode() of the STUB-backed host library, recorded call by call: the return value of every x264_encoder_encode (zeros and
errors included), x264_encoder_delayed_frames after every call, the formatted log at info level and above, the stream's SHA-256 and the hash of what run_host.py
calls `meta`.  The pictures, then flush calls while pictures are delayed, then one more flush call (a drained session answers 0).  late=K submits one more
picture after the K-th flush call, which a GOP-slot session refuses.  Prints one JSON line; tests/golden/gop_slots_parent_calls.json holds these lines as the
commit before host/gopslots.cpp printed them.  Usage: run_host_calls.py W H FRAMES SEED [late=K] key=value ...  (env X264GPU_STUB_DEVICES as run_host.py)"""
import ctypes as C
import hashlib
import json
import os
import sys

os.environ["X264_HOST_STUB"] = "1"
HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import host_lib as HL  # noqa: E402
from quality_sessions import make_logger  # noqa: E402
from synth import synth_frames  # noqa: E402


def session(w, h, n, seed, opts, late=None, preset=b"medium"):
    H = HL.H
    frames = synth_frames(w, h, n + 1, seed=seed)
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset, None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    planes = [(w * h, 0), (w * h // 4, w * h), (w * h // 4, w * h * 5 // 4)]
    stream, meta, rets, delayed = b"", [], [], []

    def call(i):          # picture i, or a flush call (None)
        nonlocal stream
        if i is not None:
            for pl, (sz, off) in enumerate(planes):
                C.memmove(pic.img.plane[pl], frames[i][off:off + sz].ctypes.data, sz)
            pic.i_pts = i
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None if i is None else C.byref(pic), C.byref(out))
        rets.append(size)
        delayed.append(H.x264_encoder_delayed_frames(h_))
        if size > 0:
            stream += C.string_at(nal[0].p_payload, size)
            meta.append((int(out.i_type), int(out.b_keyframe), int(out.i_pts), int(out.i_dts), [(int(nal[k].i_type), int(nal[k].i_ref_idc)) for k in range(nn.value)]))
    for i in range(n):
        call(i)
    flushes = 0
    while H.x264_encoder_delayed_frames(h_) and flushes < n + 8:
        call(None)
        flushes += 1
        if late == flushes: call(n)
    call(None)
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return {"rets": rets, "delayed": delayed, "log": [[lvl, text] for lvl, text in log], "sha": hashlib.sha256(stream).hexdigest(),
            "meta": hashlib.sha256(json.dumps(meta).encode()).hexdigest()}


if __name__ == "__main__":
    w, h, n, seed = (int(x) for x in sys.argv[1:5])
    opts = {}
    for a in sys.argv[5:]:
        k, eq, v = a.partition("=")
        opts[k] = v if eq else None
    late = opts.pop("late", None)
    print(json.dumps(session(w, h, n, seed, opts, None if late is None else int(late))))

#!/usr/bin/env python3
"""N sessions with lookaheads of their own (macroblock-tree, --aq-mode 2 / 3, --direct temporal) in N threads under X264GPU_BATCH=N over the stand-in device — which
has no x264gpu_gather_rows: the group copies its members' rows one by one — then the same sessions one after the other without it.  Prints one JSON line
{"equal": [...], "sizes": [...], "distinct": n, "types": "...", "log": [[...], ...] (the batched sessions' log lines), "eff": [{"mbtree", "aq_mode", "direct"}, ...]}.
Usage: run_host_batch_side.py N W H FRAMES key=value ..."""
import ctypes as C
import json
import os
import sys
import threading

HERE = os.path.dirname(os.path.abspath(__file__))
os.environ["X264_HOST_STUB"] = "1"
sys.path.insert(0, os.path.dirname(HERE))
sys.path.insert(0, os.path.dirname(os.path.dirname(HERE)))
import host_lib as HL  # noqa: E402
from quality_sessions import make_logger  # noqa: E402
from synth import synth_frames  # noqa: E402


def session(w, h, frames, opts, out, idx, errs):
    try:
        H = HL.H
        p = HL.Param()
        assert H.x264_param_default_preset(C.byref(p), b"medium", None) == 0
        p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
        p.i_fps_num, p.i_fps_den = 25, 1
        for k, v in opts.items():
            assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
        log = []
        cb = make_logger(log)
        p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2
        p.b_annexb, p.b_repeat_headers = 1, 1
        h_ = H.x264_encoder_open_157(C.byref(p))
        assert h_, log
        eff = HL.Param()
        H.x264_encoder_parameters(h_, C.byref(eff))
        pic, po = HL.Picture(), HL.Picture()
        assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
        nal, nn = C.POINTER(HL.Nal)(), C.c_int()
        stream, types = b"", []
        for i, f in enumerate(frames):
            C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
            pic.i_pts = i
            size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(po))
            if size < 0:
                H.x264_encoder_close(h_)
                raise RuntimeError(f"encode failed: {log[-3:]}")
            if size:
                stream += C.string_at(nal[0].p_payload, size); types.append(po.i_type)
        while H.x264_encoder_delayed_frames(h_):
            size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(po))
            if size <= 0:
                H.x264_encoder_close(h_)
                raise RuntimeError(f"flush failed: {log[-3:]}")
            stream += C.string_at(nal[0].p_payload, size); types.append(po.i_type)
        H.x264_encoder_close(h_)
        out[idx] = dict(stream=stream, types=types, log=[t for _, t in log],
                        eff=dict(mbtree=eff.rc.b_mb_tree, aq_mode=eff.rc.i_aq_mode, direct=eff.analyse.i_direct_mv_pred, lookahead=eff.rc.i_lookahead))
    except Exception as e:  # noqa: BLE001
        errs[idx] = f"session {idx}: {e!r}"


def main():
    n, w, h, nf = (int(x) for x in sys.argv[1:5])
    opts = {}
    for a in sys.argv[5:]:
        k, sep, v = a.partition("=")
        opts[k] = v if sep else None
    clips = [synth_frames(w, h, nf, seed=100 + s) for s in range(n)]
    batched, solo, errs, errs_solo = [None] * n, [None] * n, [None] * n, [None] * n
    os.environ["X264GPU_BATCH"] = str(n)
    ths = [threading.Thread(target=session, args=(w, h, clips[s], opts, batched, s, errs)) for s in range(n)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    del os.environ["X264GPU_BATCH"]
    assert not any(errs), errs
    for s in range(n):
        session(w, h, clips[s], opts, solo, s, errs_solo)
    assert not any(errs_solo), errs_solo
    TYPE = {1: "I", 2: "i", 3: "P", 4: "R", 5: "B"}
    print(json.dumps({"equal": [batched[s]["stream"] == solo[s]["stream"] for s in range(n)], "sizes": [len(b["stream"]) for b in batched],
                      "distinct": len({b["stream"] for b in batched}), "types": "".join(TYPE[t] for t in batched[0]["types"]),
                      "log": [b["log"] for b in batched], "eff": [b["eff"] for b in batched], "solo_eff": [b["eff"] for b in solo]}))


main()

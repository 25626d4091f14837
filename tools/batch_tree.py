#!/usr/bin/env python3
"""The cross-session batcher with and without macroblock-tree: N sessions (default 64) at 1280x720, CRF 23 on preset medium with --b-adapt 0 --scenecut 0, every
session fed host pictures from a thread of its own through x264_encoder_encode, in ONE group (X264GPU_BATCH=N) — once with the tree (medium's default, rc-lookahead
40: every member runs its own lookahead), once with --no-mbtree.  Prints one JSON line a run: frames/s over first open .. last close, the spans, bytes a frame.
X264GPU_BATCH_TIMING=1 / X264GPU_HOST_TIMING=1 in the environment add the library's own accounts on stderr (the latter: slice-type analysis a picture, per session).
usage: batch_tree.py [sessions] [frames each] [further x264 options key=value ...]"""
import ctypes as C
import json
import os
import sys
import threading
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from x264vfw_amd import host_api as HL  # noqa: E402
from x264vfw_amd.synth import synth_frames  # noqa: E402

H = HL.H
W, HT = 1280, 720


def session(frames, n, opts, res, idx):
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", None) == 0
    p.i_width, p.i_height, p.i_csp = W, HT, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den, p.i_log_level = 25, 1, -1
    for k, v in opts:
        assert H.x264_param_parse(C.byref(p), k.encode(), v.encode() if v is not None else None) == 0, (k, v)
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    t_open = time.perf_counter()
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, W, HT) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    got = total = 0
    for i in range(n):
        f = frames[(i + idx) % len(frames)]
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out))
        assert size >= 0
        got += size > 0; total += size
    while H.x264_encoder_delayed_frames(h_):
        size = H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out))
        assert size > 0
        got += 1; total += size
    t_coded = time.perf_counter()
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    res[idx] = dict(got=got, bytes=total, t_open=t_open, t_coded=t_coded, mbtree=eff.rc.b_mb_tree, lookahead=eff.rc.i_lookahead)


def run(ns, n, opts, frames):
    os.environ["X264GPU_BATCH"] = str(ns)
    res = [None] * ns
    t0 = time.perf_counter()
    ths = [threading.Thread(target=session, args=(frames, n, opts, res, s)) for s in range(ns)]
    for t in ths:
        t.start()
    for t in ths:
        t.join()
    t1 = time.perf_counter()
    assert all(r and r["got"] == n for r in res), "a session failed"
    setup, coded = max(r["t_open"] for r in res) - t0, max(r["t_coded"] for r in res) - t0
    return {"sessions": ns, "frames_each": n, "mbtree": res[0]["mbtree"], "rc_lookahead": res[0]["lookahead"], "fps": round(ns * n / (t1 - t0), 2),
            "fps_coding_span": round(ns * n / (coded - setup), 2), "setup_s": round(setup, 2), "coding_s": round(coded - setup, 2), "teardown_s": round(t1 - t0 - coded, 2),
            "kB_per_frame": round(sum(r["bytes"] for r in res) / (ns * n) / 1e3, 2)}


def main():
    ns = int(sys.argv[1]) if len(sys.argv) > 1 else 64
    n = int(sys.argv[2]) if len(sys.argv) > 2 else 60
    extra = [(a.partition("=")[0], a.partition("=")[2] if "=" in a else None) for a in sys.argv[3:]]
    base = [("crf", "23"), ("b-adapt", "0"), ("scenecut", "0"), ("threads", "1")] + extra
    frames = synth_frames(W, HT, 16, seed=1)
    for name, opts in (("mbtree", base), ("no-mbtree", base + [("no-mbtree", None)])):
        print(json.dumps(dict(run=name, **run(ns, n, opts, frames))), flush=True)


if __name__ == "__main__":
    main()

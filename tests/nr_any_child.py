#!/usr/bin/env python3
"""One preset's --nr session through x264_encoder_encode in a process of its own, so that X264GPU_NR_ANY comes from the caller's environment (the sessions read
it when they open; tests/test_gpu_nr_any.py sets it or leaves it out).  The same noisy static content is coded at nr NR twice and at nr 0 once; the records of
the first and the last run are kept through X264GPU_DUMP_RECORDS in DIR/nr and DIR/plain and counted here.
Usage: nr_any_child.py DIR PRESET TUNE(- for none) NR [open]   -> one JSON line.  `open`: the session is opened and closed only (what it reports and logs)"""
import ctypes as C
import json
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
for k in ("X264_HOST_STUB", "X264GPU_HOST_LIB", "X264GPU_LIB", "X264GPU_BATCH"):
    os.environ.pop(k, None)
import host_lib as HL  # noqa: E402
import oracle_lib as O  # noqa: E402
from quality_sessions import make_logger  # noqa: E402
from synth import synth_frames  # noqa: E402

H = HL.H
W, HGT, NFRAMES = 96, 80, 8
NMB = (W // 16) * (HGT // 16)
LEVELS = 416          # X264GPU_MB_LEVELS


def static_frames(w, h, n, seed, noise):
    """one picture of the project's synthetic content, fresh noise of +-noise on every frame's luma, +-1 on chroma (test_gpu_b_pred_reuse.static_frames)"""
    rng = np.random.default_rng(seed)
    base = synth_frames(w, h, 1, seed=seed)[0].astype(np.int32)
    amp = np.concatenate([np.full(w * h, noise), np.full(w * h // 2, 1)])
    return [np.clip(base + rng.integers(-amp, amp + 1), 16, 235).astype(np.uint8) for _ in range(n)]


def session(preset, tune, nr, frames, dump=None):
    """-> dict(nr reported, log, stream, decoded: every picture of the stream decodes on the checker to the session's reconstruction)"""
    if dump:
        os.makedirs(dump)
        os.environ["X264GPU_DUMP_RECORDS"] = dump
    else:
        os.environ.pop("X264GPU_DUMP_RECORDS", None)
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset.encode(), None if tune == "-" else tune.encode()) == 0
    p.i_width, p.i_height, p.i_csp, p.i_fps_num, p.i_fps_den = W, HGT, HL.X264_CSP_I420, 25, 1
    assert H.x264_param_parse(C.byref(p), b"nr", str(nr).encode()) == 0
    log = []
    cb = make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2
    p.b_vfr_input, p.b_annexb, p.b_repeat_headers = 0, 1, 1
    h = H.x264_encoder_open_157(C.byref(p))
    assert h, "x264_encoder_open failed"
    eff = HL.Param()
    H.x264_encoder_parameters(h, C.byref(eff))
    res = dict(nr=int(eff.analyse.i_noise_reduction), log=log, stream=b"", decoded=None, bframes=int(eff.i_bframe), cabac=int(eff.b_cabac))
    if frames is None:
        H.x264_encoder_close(h)
        return res
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, W, HGT) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    recons = []

    def take(size):
        assert size >= 0, "x264_encoder_encode failed"
        if size:
            res["stream"] += C.string_at(nal[0].p_payload, size)
            rec = np.zeros(W * HGT * 3 // 2, np.uint8)
            assert H.x264host_get_recon(h, rec.ctypes.data) == 0
            recons.append(rec)
    for i, f in enumerate(frames):
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        take(H.x264_encoder_encode(h, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out)))
    while H.x264_encoder_delayed_frames(h):
        take(H.x264_encoder_encode(h, C.byref(nal), C.byref(nn), None, C.byref(out)))
    H.x264_encoder_close(h)
    H.x264_picture_clean(C.byref(pic))
    dec = O.h264_decode(res["stream"], len(frames), W, HGT)
    res["decoded"] = len(dec) == len(recons) == len(frames) and all(np.array_equal(d, r) for d, r in zip(dec, recons))
    return res


def inter_levels(dump):
    """(non-zero levels of the inter macroblocks, inter macroblocks that are no skips) over the pictures dumped in `dump`"""
    n = inter = 0
    names = sorted(os.listdir(dump))
    assert len(names) == NFRAMES, names
    for name in names:
        raw = np.fromfile(os.path.join(dump, name), np.uint8)
        head = raw.size - NMB * (O.MB_DTYPE.itemsize + LEVELS * 2 + 4)          # x264gpu_pic in front, the quantiser offsets behind
        assert head > 0
        mbs = raw[head:head + NMB * O.MB_DTYPE.itemsize].view(O.MB_DTYPE)
        lv = raw[head + NMB * O.MB_DTYPE.itemsize:head + NMB * (O.MB_DTYPE.itemsize + LEVELS * 2)].view(np.int16).reshape(NMB, LEVELS)
        sel = mbs["type"] >= O.MB_P_L0
        n += int(np.count_nonzero(lv[sel]))
        inter += int((sel & (mbs["type"] != O.MB_P_SKIP) & (mbs["type"] != O.MB_B_SKIP)).sum())
    return n, inter


def main():
    d, preset, tune, nr = sys.argv[1], sys.argv[2], sys.argv[3], int(sys.argv[4])
    if len(sys.argv) > 5 and sys.argv[5] == "open":
        r = session(preset, tune, nr, None)
        print(json.dumps(dict(nr=r["nr"], log=r["log"])))
        return
    frames = static_frames(W, HGT, NFRAMES, 40, 12)          # (at +-4 a CRF 23 session of this size skips nearly every macroblock: nothing to denoise)
    a = session(preset, tune, nr, frames, dump=os.path.join(d, "nr"))
    b = session(preset, tune, nr, frames)
    c = session(preset, tune, 0, frames, dump=os.path.join(d, "plain"))
    la, ia = inter_levels(os.path.join(d, "nr"))
    lc, ic = inter_levels(os.path.join(d, "plain"))
    print(json.dumps(dict(nr=a["nr"], log=a["log"], decoded=a["decoded"], same=a["stream"] == b["stream"] and len(a["stream"]) > 0, bframes=a["bframes"], cabac=a["cabac"],
                          plain_nr=c["nr"], plain_decoded=c["decoded"], levels_nr=la, levels_plain=lc, inter_nr=ia, inter_plain=ic)))


if __name__ == "__main__":
    main()

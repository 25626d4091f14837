#!/usr/bin/env python3
"""Times the macroblock-tree statistics file's share of a picture with device events (csrc/mbtree_stats.hip): x264gpu_mbtree_pack + the download of the words (a
first pass, per kept picture) and the upload of the words + x264gpu_mbtree_unpack (a second pass), beside the encode of a P picture of the same size
(x264gpu_encode_frames at the medium toolset: the macroblock loop x264gpu_encode_pictures runs too).  Median of the timed calls, one JSON line.  The measurement
runs in a child process under its own time limit; a child that fails or is cut off ends the tool with its status.
Usage: mbtree_stats_time.py [--size 1920x1080] [--calls 9] [--warmup 2] [--limit 240]"""
import argparse
import ctypes as C
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def child(a):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    import numpy as np
    import torch
    from x264vfw_amd import lib
    import oracle_lib as O
    from synth import synth_frames
    w, h = (int(x) for x in a.size.split("x"))
    n = ((w + 15) // 16) * ((h + 15) // 16)
    d_off = (torch.rand(n, device="cuda") * 16 - 8).float()
    d_words = torch.zeros(n, dtype=torch.int16, device="cuda")
    h_words = torch.zeros(n, dtype=torch.int16).pin_memory()
    d_back = torch.zeros(n, dtype=torch.float32, device="cuda")
    st = torch.cuda.current_stream().cuda_stream

    def write_side():
        lib.check(lib.x264gpu_mbtree_pack(d_off.data_ptr(), n, d_words.data_ptr(), st), "mbtree_pack")
        h_words.copy_(d_words, non_blocking=True)

    def read_side():
        d_words.copy_(h_words, non_blocking=True)
        lib.check(lib.x264gpu_mbtree_unpack(d_words.data_ptr(), n, d_back.data_ptr(), st), "mbtree_unpack")

    frames = synth_frames(w, h, 2, seed=7)
    cfg = O.default_config(w, h, refs=2, partitions=7, dct8x8=1, chroma_me=1, mixed_refs=1, cabac=1, rd=1, subme=7, psy=1, psy_rd_q8=256, chroma_qp_offset=-2, trellis=63)
    enc = C.c_void_p()
    lib.check(lib.x264gpu_encoder_create(C.byref(enc), C.byref(cfg)), "encoder_create")
    nmb = lib.x264gpu_encoder_mb_count(enc)
    d_mb = torch.zeros((nmb, 64), dtype=torch.uint8, device="cuda")
    d_lv = torch.zeros((nmb, lib.MB_LEVELS), dtype=torch.int16, device="cuda")
    d_in = [torch.from_numpy(np.ascontiguousarray(f)).cuda() for f in frames]
    lib.check(lib.x264gpu_encode_frames(enc, d_in[0].data_ptr(), 2, d_mb.data_ptr(), d_lv.data_ptr(), st), "encode_frames (I)")

    def encode_p():
        lib.check(lib.x264gpu_encode_frames(enc, d_in[1].data_ptr(), 0, d_mb.data_ptr(), d_lv.data_ptr(), st), "encode_frames (P)")

    def timed(fn):
        for _ in range(a.warmup):
            fn()
        torch.cuda.synchronize()
        ms = []
        for _ in range(a.calls):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            torch.cuda.synchronize()
            ms.append(e0.elapsed_time(e1))
        ms.sort()
        return {"median_ms": round(ms[len(ms) // 2], 4), "min_ms": round(ms[0], 4), "max_ms": round(ms[-1], 4)}
    res = {"tool": "mbtree_stats_time", "size": a.size, "macroblocks": n, "calls": a.calls, "pack_and_download": timed(write_side), "upload_and_unpack": timed(read_side),
           "encode_p_picture": timed(encode_p)}
    assert np.array_equal(d_back.cpu().numpy(), (h_words.numpy().view(np.uint16).view(">i2").astype(np.float32) / 256))
    lib.x264gpu_encoder_destroy(enc)
    print(json.dumps(res))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--size", default="1920x1080")
    ap.add_argument("--calls", type=int, default=9)
    ap.add_argument("--warmup", type=int, default=2)
    ap.add_argument("--limit", type=int, default=240, help="seconds the measuring child may take")
    ap.add_argument("--child", action="store_true")
    a = ap.parse_args()
    if a.child:
        return child(a)
    assert a.calls >= 5 and a.warmup >= 1
    cmd = ["timeout", "-k", "10", str(a.limit), sys.executable, os.path.abspath(__file__), "--child"] + [x for x in sys.argv[1:] if x != "--child"]
    sys.exit(subprocess.call(cmd))


if __name__ == "__main__":
    main()

"""What QP-RD (x264 --subme 10; cfg.qp_rd) costs a picture: one small batch of I, P, B-reference and b pictures (x264gpu_encode_pictures, re-issued: a re-issued picture
is exact) at subme 9 and at subme 10 on the same content and the same per-macroblock quantiser offsets, timed with device events around the call; and from the log
(x264gpu_encoder_set_qprd_log) the mean number of encodes a walk asked for per macroblock, by picture type.  A library without the QP-RD entries (an older build) is
timed at subme 9 alone.
usage: qprd_time.py [--streams N] [--reps N] [--size WxH] [--me 1|2]"""
import argparse, ctypes as C, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
from x264vfw_amd import lib
from x264vfw_amd.synth import synth_frames

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=8); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--size", default="640x368"); ap.add_argument("--me", type=int, default=2)
a = ap.parse_args()
W, H = (int(x) for x in a.size.split("x")); S = a.streams
has_qprd = "qp_rd" in [f[0] for f in lib.Config._fields_] and hasattr(lib, "QPRD_LOG_WORDS")
kw = dict(width=W, height=H, streams=S, refs=3, dpb=4, weightb=1, qp_i=22, qp_p=24, me_range=16, subme=9, deblock=1, deadzone_inter=21, deadzone_intra=11, dct_decimate=1,
          partitions=7, dct8x8=1, me_method=a.me, chroma_me=1, mixed_refs=1, aq_strength=1.0397, fast_pskip=1, cabac=1, rd=63 | 64, psy=1, psy_rd_q8=256, chroma_qp_offset=-2, trellis=127)
frames = [synth_frames(W, H, 4, seed=7 + s) for s in range(S)]
d_in = [torch.from_numpy(np.stack([frames[s][i] for s in range(S)])).cuda() for i in range(4)]
# coding order I (display 0), P (3), B reference (1: between 0 and 3), b (2: between the B reference and the P picture)
pics = [("I", 0, lib.make_pic(2, 22, 0, 0, 1)), ("P", 3, lib.make_pic(0, 24, 6, 1, 1, (0,))), ("Bref", 1, lib.make_pic(1, 25, 2, 2, 1, (0,), (1,))), ("b", 2, lib.make_pic(1, 26, 4, 3, 0, (2, 0), (1,)))]
out = {"streams": S, "size": a.size, "me": a.me, "reps": a.reps, "qprd_entries": has_qprd}
for mode in ("subme9", "subme10") if has_qprd else ("subme9",):
    cfg = lib.Config(**dict(kw, **({"qp_rd": 1, "subme": 10} if mode == "subme10" else {})))
    enc = C.c_void_p()
    lib.check(lib.x264gpu_encoder_create(C.byref(enc), C.byref(cfg)), "create")
    n = lib.x264gpu_encoder_mb_count(enc)
    d_mb = torch.zeros((S, n, 64), dtype=torch.uint8, device="cuda"); d_lv = torch.zeros((S, n, lib.MB_LEVELS), dtype=torch.int16, device="cuda")
    # offsets as AQ leaves them: a few quantisers either way, changing from macroblock to macroblock (the same in both modes)
    off = np.random.default_rng(3).integers(-3, 4, (S, n)).astype(np.float32)
    d_off = torch.from_numpy(off).cuda()
    lib.check(lib.x264gpu_encoder_set_mb_qp_offsets(enc, d_off.data_ptr()), "offsets")
    d_log = None
    if mode == "subme10":
        d_log = torch.zeros((S, n, lib.QPRD_LOG_WORDS), dtype=torch.int32, device="cuda")
        lib.check(lib.x264gpu_encoder_set_qprd_log(enc, d_log.data_ptr()), "log")
    res = {}
    for rep in range(a.reps + 1):          # (the first round warms: code objects loaded, the load-balance history of every picture kind in place)
        for name, disp, pic in pics:
            arr = (lib.Pic * S)(*[pic] * S)
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            lib.check(lib.x264gpu_encode_pictures(enc, d_in[disp].data_ptr(), arr, d_mb.data_ptr(), d_lv.data_ptr(), None), name)
            e1.record(); torch.cuda.synchronize()
            if rep:
                res.setdefault(name, {"ms": []})["ms"].append(round(e0.elapsed_time(e1), 2))
            if d_log is not None and rep == 1:
                cnt = d_log[:, :, 0].cpu().numpy()
                res[name]["calls_per_mb"] = round(float(cnt.mean()), 2); res[name]["calls_per_walked_mb"] = round(float(cnt[cnt > 0].mean()), 2) if (cnt > 0).any() else 0.0
                res[name]["walked"] = round(float((cnt > 0).mean()), 3)
                hdr = d_log[:, :, 1].cpu().numpy().view(np.uint32)
                res[name]["moved"] = round(float((((hdr >> 16) & 255) != (hdr & 255))[cnt > 0].mean()), 3) if (cnt > 0).any() else 0.0
    for name in res:
        res[name]["s_per_picture"] = round(float(np.median(res[name]["ms"])) / 1000.0, 4)
    out[mode] = res
    lib.x264gpu_encoder_destroy(enc)
if has_qprd:
    out["ratio"] = {name: round(out["subme10"][name]["s_per_picture"] / out["subme9"][name]["s_per_picture"], 2) for name in out["subme9"]}
print(json.dumps(out))

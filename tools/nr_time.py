"""What noise reduction (x264gpu_encoder_set_nr) costs a picture: the same 1080p P and B calls (x264gpu_encode_pictures, re-issued: a re-issued picture is exact) with
the denoising instantiations of the macroblock loop and with the plain ones, timed with device events around the call.  The offsets are a real session's: the
state updated (strength 600) behind a first pass over the P picture.  A library without the nr entries (an older build) is timed on the plain kernels alone.
--rd0 (no RD, subme 5) and --rd1 (RD with CAVLC bit counts) time the toolsets of x264gpu_encoder_set_nr_any, under any --me; a library without that entry: plain only.
usage: nr_time.py [--streams N] [--reps N] [--rd6 | --rd0 | --rd1] [--me 0|1|2|3]"""
import argparse, ctypes as C, json, os, sys
R = os.path.dirname(os.path.dirname(os.path.abspath(__file__))); sys.path.insert(0, R)
import numpy as np, torch
from x264vfw_amd import lib
from x264vfw_amd.synth import synth_frames

ap = argparse.ArgumentParser()
ap.add_argument("--streams", type=int, default=8); ap.add_argument("--reps", type=int, default=3); ap.add_argument("--rd6", action="store_true"); ap.add_argument("--me", type=int, default=1)
ap.add_argument("--rd0", action="store_true"); ap.add_argument("--rd1", action="store_true")
a = ap.parse_args()
assert a.rd6 + a.rd0 + a.rd1 <= 1
W, H, S = 1920, 1080, a.streams
try:
    set_nr, nr_update = lib.x264gpu_encoder_set_nr_any if a.rd0 or a.rd1 else lib.x264gpu_encoder_set_nr, lib.x264gpu_nr_update
except AttributeError:
    set_nr = nr_update = None
kw = dict(width=W, height=H, streams=S, refs=3, dpb=4, weightb=1, qp_i=20, qp_p=23, me_range=16, subme=9 if a.rd6 else 7, deblock=1, deadzone_inter=21, deadzone_intra=11, dct_decimate=1,
          partitions=7, dct8x8=1, me_method=a.me, chroma_me=1, mixed_refs=1, aq_strength=1.0397, fast_pskip=1, cabac=1, rd=63 if a.rd6 else 1, psy=1, psy_rd_q8=256,
          chroma_qp_offset=-2, trellis=127 if a.rd6 else 63)
if a.rd0: kw.update(subme=5, rd=0, trellis=0, psy=0, psy_rd_q8=0)
if a.rd1: kw.update(cabac=0, trellis=0)
if a.me == 3: kw.update(me_range=8)
cfg = lib.Config(**kw)
enc = C.c_void_p()
lib.check(lib.x264gpu_encoder_create(C.byref(enc), C.byref(cfg)), "create")
n = lib.x264gpu_encoder_mb_count(enc)
d_mb = torch.zeros((S, n, 64), dtype=torch.uint8, device="cuda"); d_lv = torch.zeros((S, n, lib.MB_LEVELS), dtype=torch.int16, device="cuda")
frames = [synth_frames(W, H, 3, seed=7 + s) for s in range(S)]
d_in = [torch.from_numpy(np.stack([frames[s][i] for s in range(S)])).cuda() for i in range(3)]
pics = {"I": (0, lib.make_pic(2, 20, 0, 0, 1)), "P": (2, lib.make_pic(0, 23, 4, 1, 1, (0,))), "B": (1, lib.make_pic(1, 25, 2, 2, 0, (0,), (1,)))}
d_off = torch.zeros((S, 192), dtype=torch.int16, device="cuda"); d_pic = torch.zeros((S, 1552), dtype=torch.uint8, device="cuda"); d_state = torch.zeros((S, 1552), dtype=torch.uint8, device="cuda")


def issue(name):
    disp, pic = pics[name]
    arr = (lib.Pic * S)(*[pic] * S)
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    lib.check(lib.x264gpu_encode_pictures(enc, d_in[disp].data_ptr(), arr, d_mb.data_ptr(), d_lv.data_ptr(), None), name)
    e1.record(); torch.cuda.synchronize()
    return e0.elapsed_time(e1)


issue("I")
if set_nr:          # a real session's offsets: the state behind the P picture at strength 600
    lib.check(set_nr(enc, d_off.data_ptr(), d_pic.data_ptr()), "set_nr"); issue("P")
    lib.check(nr_update(d_off.data_ptr(), d_state.data_ptr(), d_pic.data_ptr(), S, 600, None), "nr_update"); torch.cuda.synchronize()
    lib.check(set_nr(enc, None, None), "set_nr off")
out = {"streams": S, "rd": 6 if a.rd6 else 0 if a.rd0 else 1 if a.rd1 else 3, "me": a.me, "reps": a.reps, "nr_entries": bool(set_nr)}
for name in ("P", "B"):
    issue(name)          # (warm: code objects loaded, the load-balance history of this picture kind in place)
    ms = {"plain": [], "nr": []}
    for r in range(a.reps):
        for mode in ("plain", "nr") if set_nr else ("plain",):
            if set_nr: lib.check(set_nr(enc, *((d_off.data_ptr(), d_pic.data_ptr()) if mode == "nr" else (None, None))), "set_nr")
            ms[mode].append(issue(name))
    if set_nr: lib.check(set_nr(enc, None, None), "set_nr off")
    out[name] = {k: [round(x, 2) for x in v] for k, v in ms.items() if v}
    if ms["nr"]: out[name]["ratio_of_medians"] = round(float(np.median(ms["nr"]) / np.median(ms["plain"])), 4)
print(json.dumps(out))
lib.x264gpu_encoder_destroy(enc)

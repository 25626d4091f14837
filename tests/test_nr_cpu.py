"""--nr without a GPU: (1) the twin (tests/nr_ref.py) against known answers, (2) the new entries are declared, bound and built, (3) the host's rules over the CPU
stand-in of the device library, which has no nr entries: the session warns once, runs nr 0 and codes what it codes without the option."""
import json
import os
import re
import subprocess
import sys

import numpy as np

import nr_ref as N

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_zero_state_gives_zero_offsets():
    for strength in (0, 1, 600, 65536):
        st = N.zero_state()
        assert not N.update(st, None, strength).any()
        assert st == N.zero_state()
        assert not N.update(st, N.zero_state(), strength).any()


def test_dc_is_never_denoised():
    rng = np.random.default_rng(1)
    st = N.zero_state()
    for _ in range(4):
        pic = {"sum": [[int(v) for v in rng.integers(0, 1 << 22, 64)] for _ in range(3)], "count": [int(v) for v in rng.integers(1, 5000, 3)]}
        off = N.update(st, pic, 600)
        assert (off[:, 0] == 0).all() and off[1, 1:].any() and off[0, 1:16].any() and off[2, 1:16].any()
        assert not off[0, 16:].any() and not off[2, 16:].any(), "categories 0 and 2 have 16 entries"


def test_one_update_worked_by_hand():
    """strength 100, category 0, count 10 blocks.  Index 1 (one odd coordinate, weight2 320): sum 400 -> (100 * 10 + 400 // 2) // (400 * 320 // 256 + 1) =
    1200 // 501 = 2.  Index 5 (both odd, 128): sum 90 -> (1000 + 45) // (90 * 128 // 256 + 1) = 1045 // 46 = 22.  Index 2 (both even, 800): sum 37 ->
    (1000 + 18) // (37 * 800 // 256 + 1) = 1018 // 116 = 8.  Category 1, count 3, index 9 (row 1, column 1: class 1, weight2 201): sum 1000 ->
    (300 + 500) // (1000 * 201 // 256 + 1) = 800 // 786 = 1.  An index whose sum is 0: strength * count // 1 = 1000."""
    pic = N.zero_state()
    pic["count"] = [10, 3, 0]
    pic["sum"][0][1], pic["sum"][0][5], pic["sum"][0][2], pic["sum"][1][9] = 400, 90, 37, 1000
    st = N.zero_state()
    off = N.update(st, pic, 100)
    assert (int(off[0][1]), int(off[0][5]), int(off[0][2]), int(off[1][9]), int(off[0][3]), int(off[0][0])) == (2, 22, 8, 1, 1000, 0)
    assert N.weight2(0, 1) == 320 and N.weight2(0, 5) == 128 and N.weight2(0, 2) == 800 and N.weight2(1, 9) == 201 and N.weight2(1, 0) == 256
    assert st["count"] == [10, 3, 0] and st["sum"][0][1] == 400
    assert not off[2].any(), "a category without blocks keeps zero offsets"


def test_halving_at_the_thresholds():
    for cat in range(3):
        thr = (1 << 16) if cat == 1 else (1 << 18)
        for count, halved in ((thr, False), (thr + 1, True)):
            st = N.zero_state()
            st["count"][cat] = count
            st["sum"][cat][3] = 1001
            N.update(st, None, 10)
            assert st["count"][cat] == (count >> 1 if halved else count), (cat, count)
            assert st["sum"][cat][3] == (500 if halved else 1001)


def test_offsets_are_clamped_to_32767():
    st = N.zero_state()
    st["count"][0] = 1000
    off = N.update(st, None, 65536)          # sums 0: 65 536 000 // 1
    assert (off[0, 1:16] == 32767).all() and off[0, 0] == 0
    st["sum"][0][1] = 100                    # 65 536 050 // 126 = 520 127: still clamped
    assert int(N.update(st, None, 65536)[0][1]) == 32767


def test_denoise_with_zero_offsets_is_the_identity_and_sums():
    rng = np.random.default_rng(2)
    for cat in range(3):
        blocks = rng.integers(-32768, 32768, (5, N.NCOEF[cat])).astype(np.int16)
        out, sums = N.denoise_blocks(blocks, cat, N.zero_offsets())
        assert np.array_equal(out, blocks)
        assert sums["sum"][cat][:N.NCOEF[cat]] == [int(v) for v in np.abs(blocks.astype(np.int64)).sum(axis=0)]
        assert sums["count"] == [5 if c == cat else 0 for c in range(3)]


def test_an_offset_above_the_coefficient_gives_zero_never_a_sign_flip():
    off = N.zero_offsets()
    off[0][:16] = [0, 5, 5, 5, 100, 100, 100, 100, 32767, 32767, 32767, 32767, 1, 1, 1, 1]
    blk = np.array([-7, 4, -4, 9, -99, 100, -101, 150, 32767, -32767, -32768, 12, 1, -1, 2, -2], np.int16)
    out = N.denoise(blk, 0, off)
    assert out.tolist() == [-7, 0, 0, 4, 0, 0, -1, 50, 0, 0, -1, 0, 0, 0, 1, -1]
    assert all(int(a) * int(b) >= 0 for a, b in zip(out, blk))


def test_update_chain_crosses_both_thresholds():
    """the chain tests/test_gpu_nr.py hands the device: both halving rules fire on the way"""
    import test_gpu_nr as G
    fired = set()
    for s in range(2):
        st = N.zero_state()
        for pic in G.update_chain(s):
            before = list(st["count"])
            N.update(st, pic, 600)
            for cat in range(3):
                if st["count"][cat] < before[cat] + pic["count"][cat]:
                    fired.add((s, cat))
    assert {(0, 0), (0, 1), (1, 1), (1, 2)} <= fired, fired


def test_header_declares_binding_exports_and_library_holds_the_entries():
    names = ("x264gpu_encoder_set_nr", "x264gpu_nr_update", "x264gpu_denoise_blocks")
    hdr = open(os.path.join(ROOT, "include", "x264gpu.h")).read()
    for name in names:
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/x264gpu.h"
    assert "x264host_nr_offsets" in open(os.path.join(ROOT, "include", "x264gpu_host.h")).read()
    import ctypes as C
    from x264vfw_amd import lib
    for name in names:
        assert name in lib.EXPORTS
    assert C.sizeof(lib.NrOffsets) == 384 and C.sizeof(lib.NrSums) == 1552
    so = C.CDLL(os.path.join(ROOT, "x264vfw_amd", "libx264gpu.so"))
    for name in names:
        assert hasattr(so, name), f"libx264gpu.so lacks {name}"


_CHILD = r"""
import ctypes as C, json, os, sys
os.environ["X264_HOST_STUB"] = "1"
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import host_lib as HL
import quality_sessions as S
from synth import synth_frames
H = HL.H
frames = synth_frames(64, 48, 5, seed=5)
base = {"qp": 26, "keyint": 30, "bframes": 2, "b-adapt": 0, "me": "hex", "subme": 7, "trellis": 1}
out = {}
def eff_nr(opts):
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", None) == 0
    p.i_width, p.i_height, p.i_csp, p.i_fps_num, p.i_fps_den = 64, 48, HL.X264_CSP_I420, 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = S.make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2
    h = H.x264_encoder_open_157(C.byref(p))
    assert h
    eff = HL.Param()
    H.x264_encoder_parameters(h, C.byref(eff))
    offs = (C.c_uint16 * 192)()
    rc = H.x264host_nr_offsets(h, offs)
    H.x264_encoder_close(h)
    return {"nr": eff.analyse.i_noise_reduction, "log": log, "hook": rc, "offs_any": any(offs)}
runs = [S.run_session(64, 48, frames, dict(base, **extra), quality=False, log_level=2, want_recon=False) for extra in ({}, {"nr": 200})]
out["equal"] = runs[0]["stream"] == runs[1]["stream"] and len(runs[0]["stream"]) > 0
out["log"] = [r["log"] for r in runs]
out["plain"] = eff_nr(dict(base, nr=200))
for name, extra in (("no-cabac", {"no-cabac": None}), ("me=dia", {"me": "dia"}), ("subme=5", {"subme": 5}), ("trellis=0", {"trellis": 0}), ("threads=4", {"threads": 4, "bframes": 0})):
    out[name] = eff_nr(dict(base, nr=200, **extra))
print(json.dumps(out))
"""


def _nr_warnings(log):
    return [t for lvl, t in log if lvl == 1 and "nr (noise reduction)" in t]


def test_host_over_the_stand_in_warns_once_and_runs_nr_0():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    r = subprocess.run([sys.executable, "-c", _CHILD, HERE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    out = json.loads(r.stdout.strip().splitlines()[-1])
    assert out["equal"], "nr=200 over a device library without the entries must code the bytes of the session without it"
    assert len(_nr_warnings(out["log"][1])) == 1 and not _nr_warnings(out["log"][0]), out["log"]
    assert out["plain"]["nr"] == 0 and len(_nr_warnings(out["plain"]["log"])) == 1 and out["plain"]["hook"] == -1 and not out["plain"]["offs_any"]
    for name in ("no-cabac", "me=dia", "subme=5", "trellis=0", "threads=4"):
        assert out[name]["nr"] == 0 and len(_nr_warnings(out[name]["log"])) == 1, (name, out[name]["log"])

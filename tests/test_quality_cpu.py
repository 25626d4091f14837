"""--psnr / --ssim without a GPU: the numpy reference's own checks, the host's pure figures through the stub-built host library, the ABI, and a stub
session with the flags set (the stand-in device library has no quality entry: the session must run exactly as without them)."""
import json
import os
import re
import subprocess
import sys

import numpy as np
import pytest

import quality_ref as Q

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def _pic(w, h, seed):
    return np.random.default_rng(seed).integers(0, 256, w * h * 3 // 2, dtype=np.uint8)


def test_reference_constants():
    assert (Q.C1, Q.C2) == (416, 235963)


@pytest.mark.parametrize("w,h,cnt", [(1920, 1080, 128104), (352, 288, 6020), (66, 50, 165)])
def test_reference_window_counts(w, h, cnt):
    assert Q.ssim_count(w, h) == cnt
    if w < 1000:
        a = _pic(w, h, 1)
        assert Q.quality(a, a, w, h)["ssim_cnt"] == cnt


@pytest.mark.parametrize("w,h", [(64, 48), (66, 50), (350, 270)])
def test_reference_identical_pictures(w, h):
    a = _pic(w, h, 2)
    r = Q.quality(a, a.copy(), w, h)
    assert r["ssd"] == [0, 0, 0]
    assert r["ssim"] == 1.0 and np.all(Q.ssim_windows(*[Q.planes(a, w, h)[0]] * 2) == 1.0)
    assert Q.picture_psnr(r["ssd"], w, h) == [100.0] * 4 and Q.ssim_db(r["ssim"]) == 100.0


def test_reference_against_a_plain_loop():
    """the reshape / four-neighbour form against the definition written out sample by sample"""
    w, h = 22, 18
    a, b = _pic(w, h, 3), _pic(w, h, 4)
    ya, yb = Q.planes(a, w, h)[0].astype(int), Q.planes(b, w, h)[0].astype(int)
    vals = []
    for by in range(((h - 2) >> 2) - 1):
        for bx in range(((w - 2) >> 2) - 1):
            pa, pb = ya[2 + 4 * by:10 + 4 * by, 2 + 4 * bx:10 + 4 * bx], yb[2 + 4 * by:10 + 4 * by, 2 + 4 * bx:10 + 4 * bx]
            s1, s2, ss, s12 = int(pa.sum()), int(pb.sum()), int((pa * pa + pb * pb).sum()), int((pa * pb).sum())
            v, c = ss * 64 - s1 * s1 - s2 * s2, s12 * 64 - s1 * s2
            vals.append((2 * s1 * s2 + 416) * (2 * c + 235963) / ((s1 * s1 + s2 * s2 + 416) * (v + 235963)))
    r = Q.quality(a, b, w, h)
    assert r["ssim_cnt"] == len(vals) == 12 and abs(r["ssim_sum"] - sum(vals)) < 1e-12
    assert r["ssd"][0] == int(((ya - yb) ** 2).sum())


def test_header_declares_and_binding_exports_both_entries():
    hdr = open(os.path.join(ROOT, "include", "x264gpu.h")).read()
    for name in ("x264gpu_picture_quality", "x264gpu_encoder_quality"):
        assert re.search(r"\bint\s+" + name + r"\s*\(", hdr), f"{name} is not declared in include/x264gpu.h"
    assert "#define X264GPU_ABI_VERSION 2" in hdr and "X264GPU_QUALITY_PSNR 1" in hdr and "X264GPU_QUALITY_SSIM 2" in hdr
    from x264vfw_amd import lib
    assert "x264gpu_picture_quality" in lib.EXPORTS and "x264gpu_encoder_quality" in lib.EXPORTS
    import ctypes as C
    assert C.sizeof(lib.Quality) == 40


_CHILD = r"""
import ctypes as C, json, os, sys
os.environ["X264_HOST_STUB"] = "1"
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import host_lib as HL
H = HL.H
out = {"psnr": [H.x264host_psnr(s, n) for s, n in ((0.0, 100.0), (6502500.0, 100.0), (1234567.0, 101376.0), (1e-9, 1e9))],
       "ssim_db": [H.x264host_ssim_db(v) for v in (1.0, 0.0, 0.9, 0.987654321, 1.0 - 1e-11)]}
import quality_sessions as S
from synth import synth_frames
frames = synth_frames(64, 48, 4, seed=5)
base = {"qp": 26, "keyint": 30, "bframes": 0, "weightp": 0}
runs = [S.run_session(64, 48, frames, base, quality=q, log_level=2, want_recon=False) for q in (False, True)]
out["equal"] = runs[0]["stream"] == runs[1]["stream"] and len(runs[0]["stream"]) > 0
out["rc"] = [[p["rc"] for p in r["pics"]] + [r["summary_rc"]] for r in runs]
out["log"] = [[t for _, t in r["log"]] for r in runs]
print(json.dumps(out))
"""


def _child():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    r = subprocess.run([sys.executable, "-c", _CHILD, HERE], capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.fixture(scope="module")
def child():
    return _child()


def test_host_psnr_and_ssim_db_follow_the_formulas(child):
    out = child
    want = [100.0, 0.0, -10.0 * np.log10(1234567.0 / (65025.0 * 101376.0)), 100.0]
    assert out["psnr"][0] == 100.0 and out["psnr"][3] == 100.0
    assert np.allclose(out["psnr"], want, rtol=0, atol=1e-12)
    assert np.allclose(out["psnr"], [Q.psnr(s, n) for s, n in ((0.0, 100.0), (6502500.0, 100.0), (1234567.0, 101376.0), (1e-9, 1e9))], rtol=0, atol=1e-12)
    want = [100.0, 0.0, 10.0, -10.0 * np.log10(1.0 - 0.987654321), 100.0]
    assert np.allclose(out["ssim_db"], want, rtol=0, atol=1e-9)


def test_stub_session_with_the_flags_runs_as_without(child):
    """the stand-in device library has no x264gpu_encoder_quality: the host library still loads (weak binding), warns once, codes the same bytes and reports nothing"""
    out = child
    assert out["equal"]
    assert out["rc"] == [[-1] * 5, [-1] * 5]
    warn = "psnr / ssim: the device library has no quality entry\n"
    assert out["log"][1].count(warn) == 1 and warn not in out["log"][0], out["log"]
    assert [t for t in out["log"][1] if t != warn] == out["log"][0]          # nothing else is said: no per-picture line, no summary

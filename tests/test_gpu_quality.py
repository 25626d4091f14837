"""-m gpu: --psnr / --ssim on the device.  The primitive (x264gpu_picture_quality) against the numpy reference (tests/quality_ref.py); the pipeline
(x264gpu_encoder_quality behind every picture of a session) against the same reference over the session's own reconstruction and source; no effect on the
bitstream; cross-session batches; the direction of the figures; the closing lines through the VfW driver.

Bounds: sums of squared differences and window counts are integers and must be equal.  The mean SSIM may differ from the float64 reference by 1e-6: a
window value is computed in float32 (four conversions, two products and a quotient: about five roundings of 2^-24, 3e-7 relative on values <= 1), and a
mean cannot be off by more than its worst term."""
import ctypes as C
import os
import re
import subprocess
import sys
import threading

import numpy as np
import pytest

import quality_ref as Q
from synth import synth_frames

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
SSIM_TOL = 1e-6


def _pairs(w, h, seed):
    """a random; b = a, a +- 2, a +- 20 (clipped), independent random, all-0 vs all-255"""
    rng = np.random.default_rng(seed)
    n = w * h * 3 // 2
    a = rng.integers(0, 256, n, dtype=np.uint8)
    def off(d):
        return np.clip(a.astype(np.int16) + d * rng.choice(np.array([-1, 1], np.int16), n), 0, 255).astype(np.uint8)
    return [(a, a.copy()), (a, off(2)), (a, off(20)), (a, rng.integers(0, 256, n, dtype=np.uint8)), (np.zeros(n, np.uint8), np.full(n, 255, np.uint8))]


def _run(lib, a, b, n, w, h, flags=3):
    """-> the n x264gpu_quality results as a (n, 40) byte array"""
    import torch
    da, db = torch.from_numpy(np.ascontiguousarray(a)).cuda(), torch.from_numpy(np.ascontiguousarray(b)).cuda()
    out = torch.full((n * 40,), 0xa5, dtype=torch.uint8, device="cuda")
    lib.check(lib.x264gpu_picture_quality(da.data_ptr(), db.data_ptr(), n, w, h, flags, out.data_ptr(), None), "picture_quality")
    torch.cuda.synchronize()
    return out.cpu().numpy().reshape(n, 40)


def _fields(row):
    ssd = [int(x) for x in row[:24].view(np.uint64)]
    return ssd, float(row[24:32].view(np.float64)[0]), int(row[32:36].view(np.uint32)[0]), int(row[36:40].view(np.uint32)[0])


@pytest.mark.parametrize("w,h", [(64, 48), (66, 50), (352, 288), (350, 270), (1920, 1080)])
def test_primitive_equals_the_reference(gpu, w, h):
    pairs = _pairs(w, h, 1000 + w)
    a, b = np.concatenate([p[0] for p in pairs]), np.concatenate([p[1] for p in pairs])
    got = _run(gpu, a, b, len(pairs), w, h)
    for i, (pa, pb) in enumerate(pairs):
        ref = Q.quality(pa, pb, w, h)
        ssd, ssum, cnt, pad = _fields(got[i])
        print(f"{w}x{h} pair {i}: ssd {ssd} ref {ref['ssd']}; cnt {cnt} ref {ref['ssim_cnt']}; ssim {ssum / max(cnt, 1):.9f} ref {ref['ssim']:.9f} diff {abs(ssum / max(cnt, 1) - ref['ssim']):.3e}")
        assert ssd == ref["ssd"], (i, ssd, ref["ssd"])
        assert cnt == ref["ssim_cnt"] == Q.ssim_count(w, h) and pad == 0
        assert abs(ssum / cnt - ref["ssim"]) <= SSIM_TOL, (i, ssum / cnt, ref["ssim"])
    assert _fields(got[0])[1] / _fields(got[0])[2] == 1.0          # identical pictures: every window is exactly 1
    again = _run(gpu, a, b, len(pairs), w, h)
    assert np.array_equal(got, again), "the same call twice must give identical bytes"


def test_primitive_batch_equals_single_calls(gpu):
    """n = 37 in one call agrees, stream by stream, with n = 1 (pictures of 350 x 270 x 1.5 bytes: every other one starts 2 bytes off a dword)"""
    w, h, n = 350, 270, 37
    rng = np.random.default_rng(7)
    sz = w * h * 3 // 2
    a = rng.integers(0, 256, n * sz, dtype=np.uint8)
    b = np.clip(a.astype(np.int16) + rng.integers(-9, 10, n * sz), 0, 255).astype(np.uint8)
    many = _run(gpu, a, b, n, w, h)
    for s in range(n):
        one = _run(gpu, a[s * sz:(s + 1) * sz], b[s * sz:(s + 1) * sz], 1, w, h)
        assert np.array_equal(one[0], many[s]), s
    ref = Q.quality(a[36 * sz:], b[36 * sz:], w, h)
    assert _fields(many[36])[0] == ref["ssd"] and abs(_fields(many[36])[1] / ref["ssim_cnt"] - ref["ssim"]) <= SSIM_TOL


def test_primitive_flags_and_arguments(gpu):
    w, h = 64, 48
    (a, _), (_, b) = _pairs(w, h, 5)[0], _pairs(w, h, 5)[3]
    ref = Q.quality(a, b, w, h)
    both, ps, ss = _fields(_run(gpu, a, b, 1, w, h, 3)[0]), _fields(_run(gpu, a, b, 1, w, h, 1)[0]), _fields(_run(gpu, a, b, 1, w, h, 2)[0])
    assert both[0] == ref["ssd"] and ps == (ref["ssd"], 0.0, 0, 0) and ss == ([0, 0, 0], both[1], both[2], 0)
    import torch
    d = torch.zeros(w * h * 3, dtype=torch.uint8, device="cuda")
    o = torch.zeros(40, dtype=torch.uint8, device="cuda")
    for args in ((1, w, h, 0), (1, w, h, 4), (1, 14, h, 3), (1, w, 14, 3), (1, w + 1, h, 3), (1, w, h + 1, 3), (0, w, h, 3)):
        n, ww, hh, fl = args
        assert gpu.x264gpu_picture_quality(d.data_ptr(), d.data_ptr(), n, ww, hh, fl, o.data_ptr(), None) == -1, args


def test_encoder_entry_on_several_streams(gpu):
    """x264gpu_encoder_quality directly: EINVAL before any encode call and for flags outside 1..3; then, for three streams of a 66 x 50 session (coded size
    80 x 64: only the visible samples count), the last picture's statistics against the reference over x264gpu_encoder_get_recon"""
    import oracle_lib as O
    import torch
    from gpu_enc import GpuEncoder
    w, h, S = 66, 50, 3
    g = GpuEncoder(O.default_config(w, h, streams=S))
    out = torch.zeros(S * 40, dtype=torch.uint8, device="cuda")
    assert gpu.x264gpu_encoder_quality(g.h, 3, out.data_ptr(), None) == -1
    clips = [synth_frames(w, h, 2, seed=40 + s) for s in range(S)]
    for i in range(2):
        g.encode([clips[s][i] for s in range(S)], 2 if i == 0 else 0)
        assert gpu.x264gpu_encoder_quality(g.h, 0, out.data_ptr(), None) == -1 and gpu.x264gpu_encoder_quality(g.h, 4, out.data_ptr(), None) == -1
        gpu.check(gpu.x264gpu_encoder_quality(g.h, 3, out.data_ptr(), None), "encoder_quality")
        torch.cuda.synchronize()
        got = out.cpu().numpy().reshape(S, 40)
        for s in range(S):
            ref = Q.quality(clips[s][i], g.recon(s), w, h)
            ssd, ssum, cnt, _ = _fields(got[s])
            assert ssd == ref["ssd"] and cnt == ref["ssim_cnt"] and abs(ssum / cnt - ref["ssim"]) <= SSIM_TOL, (i, s, ssd, ref)


# ---- the pipeline ----
SESSIONS = {
    "cif_medium_b": (352, 288, {"keyint": 30, "bframes": 3, "rc-lookahead": 6}, {}),                                   # medium: CRF, B pictures, b-adapt 1, pictures in flight
    "cif_medium_b_serial": (352, 288, {"keyint": 30, "bframes": 3, "rc-lookahead": 6}, {"X264GPU_INFLIGHT": "0"}),     # ... one picture a call
    "odd_medium_b": (350, 270, {"qp": 25, "keyint": 30, "bframes": 3, "scenecut": 0, "b-adapt": 0}, {}),
    "odd_medium_b_serial": (350, 270, {"qp": 25, "keyint": 30, "bframes": 3, "scenecut": 0, "b-adapt": 0}, {"X264GPU_INFLIGHT": "0"}),
    "cif_slices4": (352, 288, {"qp": 27, "keyint": 30, "bframes": 2, "slices": 4}, {}),
    "odd_cavlc_ip": (350, 270, {"qp": 26, "keyint": 6, "bframes": 0, "weightp": 0, "no-cabac": None, "scenecut": 0}, {}),
}


def _with_env(env, fn):
    old = {k: os.environ.get(k) for k in env}
    os.environ.update(env)
    try:
        return fn()
    finally:
        for k, v in old.items():
            if v is None:
                os.environ.pop(k, None)
            else:
                os.environ[k] = v


def _summary_numbers(text):
    out = {}
    for line in text.splitlines():
        m = re.match(r"frame ([IPB]):(\d+)\s+Avg QP:\s*([\d.]+)\s+size:\s*(\d+)\s+PSNR Mean Y:\s*([\d.]+) U:\s*([\d.]+) V:\s*([\d.]+) Avg:\s*([\d.]+) Global:\s*([\d.]+)$", line)
        if m:
            out[m.group(1)] = [int(m.group(2))] + [float(x) for x in m.groups()[2:]]
        m = re.match(r"SSIM Mean Y:([\d.]+) \(\s*([\d.]+)db\)$", line)
        if m:
            out["ssim"] = [float(m.group(1)), float(m.group(2))]
        m = re.match(r"PSNR Mean Y:\s*([\d.]+) U:\s*([\d.]+) V:\s*([\d.]+) Avg:\s*([\d.]+) Global:\s*([\d.]+) kb/s:([\d.]+)$", line)
        if m:
            out["psnr"] = [float(x) for x in m.groups()]
    return out


@pytest.mark.parametrize("name", list(SESSIONS))
def test_session_quality_equals_the_reference_and_leaves_the_stream_alone(gpu, name):
    import quality_sessions as S
    w, h, opts, env = SESSIONS[name]
    nfr = 12
    frames = synth_frames(w, h, nfr, seed=77)
    r = _with_env(env, lambda: S.run_session(w, h, frames, opts, quality=True, log_level=3))
    assert len(r["pics"]) == nfr
    ps_all, ss_all, ssd_all, sizes = [], [], 0, 0
    for k, p in enumerate(r["pics"]):
        assert p["rc"] == 0
        ref = Q.quality(frames[p["pts"]], p["recon"], w, h)
        ref_ps = Q.picture_psnr(ref["ssd"], w, h)
        print(f"{name} picture {k} pts {p['pts']} type {p['type']}: ssd {p['ssd']} ref {ref['ssd']}; psnr {p['psnr'][0]:.4f}; ssim {p['ssim']:.9f} ref {ref['ssim']:.9f} diff {abs(p['ssim'] - ref['ssim']):.3e}")
        assert p["ssd"] == ref["ssd"], (k, p["ssd"], ref["ssd"])
        assert np.allclose(p["psnr"], ref_ps, rtol=0, atol=1e-9), (k, p["psnr"], ref_ps)
        assert abs(p["ssim"] - ref["ssim"]) <= SSIM_TOL, (k, p["ssim"], ref["ssim"])
        ps_all.append(p["psnr"]); ss_all.append(p["ssim"]); ssd_all += sum(p["ssd"]); sizes += p["size"]
    # the closing lines: what x264_encoder_close logged is what the hook returns, and their means are the means of the per-picture values
    assert r["summary_rc"] == len(r["summary"]) > 0
    info = [t for lvl, t in r["log"] if lvl == 2]
    assert "".join(info).endswith(r["summary"]), (info[-5:], r["summary"])
    assert len([t for lvl, t in r["log"] if lvl == 3 and re.match(r"frame=\s*\d+ QP=[\d.]+ Slice:[IPB] Poc:\d+\s* size=\d+ bytes PSNR Y:\s*[\d.]+ U:\s*[\d.]+ V:\s*[\d.]+ SSIM Y:[\d.]+\n$", t)]) == nfr
    num = _summary_numbers(r["summary"])
    assert sum(num[t][0] for t in "IPB" if t in num) == nfr and "ssim" in num and "psnr" in num, r["summary"]
    mean = np.mean(np.array(ps_all), axis=0)
    assert np.allclose(num["psnr"][:4], mean, rtol=0, atol=5.1e-4), (num["psnr"], mean)
    assert abs(num["psnr"][4] - Q.psnr(ssd_all, nfr * w * h * 3 / 2)) <= 5.1e-4
    assert abs(num["psnr"][5] - sizes / nfr / 125.0 * 25.0) <= 5.1e-3
    assert abs(num["ssim"][0] - np.mean(ss_all)) <= 5.1e-8 and abs(num["ssim"][1] - Q.ssim_db(np.mean(ss_all))) <= 5.1e-4
    if name == "cif_medium_b":
        assert S.H.x264host_pictures_in_flight is not None and any(t.startswith("up to ") for _, t in r["log"]), "this session was meant to run with pictures in flight"
    # no side effect: the same session without the flags writes the same bytes, says nothing of quality and has nothing to report
    off = _with_env(env, lambda: S.run_session(w, h, frames, opts, quality=False, log_level=3, want_recon=False))
    assert off["stream"] == r["stream"]
    assert off["summary_rc"] == -1 and all(p["rc"] == -1 for p in off["pics"])
    assert not [t for _, t in off["log"] if "PSNR" in t or "SSIM" in t]


def test_parts_asked_for(gpu):
    """--psnr alone / --ssim alone: only those parts in the lines and in the hook"""
    import quality_sessions as S
    w, h = 176, 144
    frames = synth_frames(w, h, 4, seed=3)
    opts = {"qp": 26, "keyint": 30, "bframes": 0, "weightp": 0}
    both = S.run_session(w, h, frames, opts, quality=True, log_level=3, want_recon=False)
    ps = S.run_session(w, h, frames, opts, quality={"psnr": None}, log_level=3, want_recon=False)
    ss = S.run_session(w, h, frames, opts, quality={"ssim": None}, log_level=3, want_recon=False)
    for k in range(4):
        assert ps["pics"][k]["psnr"] == both["pics"][k]["psnr"] and ps["pics"][k]["ssim"] == 0.0
        assert ss["pics"][k]["ssim"] == both["pics"][k]["ssim"] and ss["pics"][k]["psnr"] == [0.0] * 4
    assert "PSNR" in ps["summary"] and "SSIM" not in ps["summary"] and "SSIM" in ss["summary"] and "PSNR" not in ss["summary"]
    assert ps["stream"] == ss["stream"] == both["stream"]


def test_gop_slot_sessions_switch_it_off(gpu):
    import quality_sessions as S
    w, h = 176, 144
    frames = synth_frames(w, h, 8, seed=4)
    r = S.run_session(w, h, frames, {"qp": 26, "keyint": 4, "bframes": 0, "weightp": 0, "threads": 2, "scenecut": 0}, quality=True, log_level=2, want_recon=False)
    assert len(r["pics"]) == 8 and all(p["rc"] == -1 for p in r["pics"]) and r["summary_rc"] == -1
    assert len([t for _, t in r["log"] if t.startswith("psnr / ssim switched off in GOP-slot sessions")]) == 1


def _batch_sessions(n, w, h, nfr, opts, batch):
    import quality_sessions as S
    clips = [synth_frames(w, h, nfr, seed=300 + s) for s in range(n)]
    res, errs = [None] * n, []

    def one(s):
        try:
            res[s] = S.run_session(w, h, clips[s], opts, quality=True, log_level=-1, want_recon=False)
        except BaseException as e:  # noqa: BLE001
            errs.append(f"session {s}: {e!r}")
    if batch:
        ths = [threading.Thread(target=one, args=(s,)) for s in range(n)]
        _with_env({"X264GPU_BATCH": str(n)}, lambda: ([t.start() for t in ths], [t.join() for t in ths]))
    else:
        for s in range(n):
            one(s)
    assert not errs, errs
    return res


@pytest.mark.parametrize("overlap", ["1", "0"])
def test_batched_sessions_report_what_they_report_alone(gpu, overlap):
    """8 sessions of different content (and so, under CRF, different quantisers) in one cross-session batch: picture by picture the same sums of squared
    differences and the same SSIM bits as each session alone"""
    n, w, h, nfr = 8, 176, 144, 9
    opts = {"crf": 24, "keyint": 8, "min-keyint": 8, "scenecut": 0, "b-adapt": 0, "bframes": 2, "no-mbtree": None}
    solo = _batch_sessions(n, w, h, nfr, opts, False)
    together = _with_env({"X264GPU_BATCH_OVERLAP": overlap}, lambda: _batch_sessions(n, w, h, nfr, opts, True))
    assert len({s["stream"] for s in solo}) == n
    for s in range(n):
        assert together[s]["stream"] == solo[s]["stream"], s
        assert len(together[s]["pics"]) == len(solo[s]["pics"]) == nfr
        for k in range(nfr):
            a, b = together[s]["pics"][k], solo[s]["pics"][k]
            assert a["rc"] == b["rc"] == 0 and a["pts"] == b["pts"]
            assert a["ssd"] == b["ssd"] and sum(a["ssd"]) > 0, (s, k)
            assert np.float64(a["ssim"]).tobytes() == np.float64(b["ssim"]).tobytes(), (s, k, a["ssim"], b["ssim"])
            assert a["psnr"] == b["psnr"]
        assert together[s]["summary"] == solo[s]["summary"]


def test_figures_fall_with_the_quantiser(gpu):
    import quality_sessions as S
    w, h = 352, 288
    frames = synth_frames(w, h, 8, seed=11)
    means = []
    for qp in (20, 30, 40):
        r = S.run_session(w, h, frames, {"qp": qp, "keyint": 30, "bframes": 3}, quality=True, log_level=-1, want_recon=False)
        means.append((np.mean([p["psnr"][0] for p in r["pics"]]), np.mean([p["ssim"] for p in r["pics"]])))
    print("mean PSNR-Y / SSIM at CQP 20, 30, 40:", means)
    assert means[0][0] > means[1][0] > means[2][0] and means[0][1] > means[1][1] > means[2][1], means


_VFW_CHILD = r"""
import ctypes as C, os, sys
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import numpy as np
import host_lib as V
from synth import synth_frames
D = V.H.DriverProc
w, h, nfr = 176, 144, 6
frames = synth_frames(w, h, nfr, seed=21)
ico = V.ICOPEN(fccType=V.fourcc(b"vidc"))
cid = D(0, None, V.DRV_OPEN, 0, V.addr(ico))
n = D(cid, None, V.ICM_GETSTATE, 0, 0)
cfg = V.VfwConfig()
D(cid, None, V.ICM_GETSTATE, V.addr(cfg), n)
cfg.i_encoding_type, cfg.i_qp, cfg.extra_cmdline = 1, 27, b"--keyint 30 --bframes 0 --weightp 0"
cfg.b_psnr, cfg.b_ssim, cfg.i_log_level = 1, 1, 3          # the driver's log level "info"
assert D(cid, None, V.ICM_SETSTATE, V.addr(cfg), n) == n
inb, outb = V.bmi(w, h, b"I420"), V.BITMAPINFO()
assert D(cid, None, V.ICM_COMPRESS_GET_FORMAT, V.addr(inb), V.addr(outb)) == V.ICERR_OK
assert D(cid, None, V.ICM_COMPRESS_BEGIN, V.addr(inb), V.addr(outb)) == V.ICERR_OK, V.H.x264vfw_shim_log(cid)
cap = outb.bmiHeader.biSizeImage
buf = C.create_string_buffer(cap)
for f in frames:
    flags = V.DWORD(0)
    outb.bmiHeader.biSizeImage = cap
    icc = V.ICCOMPRESS(lpbiOutput=C.pointer(outb.bmiHeader), lpOutput=C.cast(buf, C.c_void_p), lpbiInput=C.pointer(inb.bmiHeader), lpInput=f.ctypes.data, lpdwFlags=C.pointer(flags))
    assert D(cid, None, V.ICM_COMPRESS, V.addr(icc), C.sizeof(icc)) == V.ICERR_OK, V.H.x264vfw_shim_log(cid)
assert D(cid, None, V.ICM_COMPRESS_END, 0, 0) == V.ICERR_OK
sys.stderr.write(V.H.x264vfw_shim_log(cid).decode(errors="replace"))
assert D(cid, None, V.DRV_CLOSE, 0, 0) == 1
"""


def test_vfw_driver_logs_the_closing_lines(gpu):
    """ICM_COMPRESS through DriverProc with b_psnr = b_ssim = 1 at the driver's log level info: the session's log (written to the child's stderr) ends with the
    three kinds of closing lines"""
    # (the child binds the product's own libraries, whatever a test before this one left in the environment for the stub-backed ones)
    env = {k: v for k, v in os.environ.items() if k not in ("X264_HOST_STUB", "X264GPU_HOST_LIB", "X264GPU_LIB")}
    r = subprocess.run([sys.executable, "-c", _VFW_CHILD, HERE], capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    lines = [ln for ln in r.stderr.splitlines() if ln.strip()]
    tail = lines[-4:]
    assert re.match(r"frame I:1\s+Avg QP:\s*[\d.]+\s+size:\s*\d+\s+PSNR Mean Y:\s*[\d.]+ U:\s*[\d.]+ V:\s*[\d.]+ Avg:\s*[\d.]+ Global:\s*[\d.]+$", tail[0]), tail
    assert re.match(r"frame P:5\s+Avg QP:\s*[\d.]+\s+size:\s*\d+\s+PSNR Mean Y:\s*[\d.]+ U:\s*[\d.]+ V:\s*[\d.]+ Avg:\s*[\d.]+ Global:\s*[\d.]+$", tail[1]), tail
    assert re.match(r"SSIM Mean Y:0\.\d{7} \(\s*[\d.]+db\)$", tail[2]), tail
    assert re.match(r"PSNR Mean Y:\s*[\d.]+ U:\s*[\d.]+ V:\s*[\d.]+ Avg:\s*[\d.]+ Global:\s*[\d.]+ kb/s:[\d.]+$", tail[3]), tail

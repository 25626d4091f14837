"""VBV on the device: the contract the re-encode guard stands on (a picture may be issued twice: x264gpu_encode_pictures again with the same destination slot and
lists gives what a first call with those arguments gives), VBV sessions through libx264gpu_host.so against the same host code over the CPU checker, and the guard
itself."""
import copy
import json
import os
import subprocess
import sys

import numpy as np
import pytest

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))


def _sequence(gpu_enc_cls, cfg, frames, reissue, qp_first=30, qp=38):
    """I0 P1 P3 B2 P4 in coding order on the host's DPB model; P3 (two references) and B2 (between P1 and P3) are coded at `qp` — with reissue first at
    qp_first and then again, same x264gpu_pic, before anything else.  -> per picture (records, levels, reconstruction)"""
    import bgop
    from x264vfw_amd import host_api as HL
    enc = gpu_enc_cls(cfg)
    dpb = bgop.HostDpb(HL, 3, 1, 0, weightp=0)
    order = bgop.schedule("IPBPP", 0)
    assert [d for d, _ in order] == [0, 1, 3, 2, 4]
    out = []
    for k, (disp, pt) in enumerate(order):
        pic, _ = dpb.plan(pt, disp, bgop.follow_of(order, k))
        twice = disp in (3, 2)
        if disp == 3: assert pic.nref[0] == 2, "the P picture predicts from two references"
        if disp == 2: assert pic.nref[0] >= 1 and pic.nref[1] == 1
        base_qp = 24 if pt <= 1 else 26
        if twice and reissue:
            first = copy.copy(pic)
            first.qp, first.qpm = qp_first, float(qp_first)
            enc.encode_pics([frames[disp]], [first])
        pic.qp = qp if twice else base_qp
        pic.qpm = float(pic.qp)
        mb, lv = enc.encode_pics([frames[disp]], [pic])
        out.append((disp, mb[0].copy(), lv[0].copy(), enc.recon(0)))
        dpb.commit()
    enc.close()
    return out


@pytest.mark.parametrize("slices", [1, 3])
def test_reissued_picture_equals_a_first_issue(gpu, slices):
    """64x48 (three macroblock rows), medium toolset.  The P and the B picture issued at qp 30 and again at qp 38 give, byte for byte, the records, levels and
    reconstruction of an encoder that coded them at qp 38 the first time, and so does the P picture that follows and references the re-issued one.  With --slices 3
    the per-slice intra statistics of the speculative slice passes (the one piece of cross-call state in the macroblock launch) have seen the first issue"""
    import oracle_lib as O
    from gpu_enc import GpuEncoder
    from synth import synth_frames
    w, h = 64, 48
    frames = synth_frames(w, h, 5, seed=11)
    kw = dict(refs=3, dpb=4, weightb=1, partitions=7, dct8x8=1, chroma_me=1, mixed_refs=1, cabac=1, rd=1, subme=7, psy=1, psy_rd_q8=256, chroma_qp_offset=-2, trellis=63)
    if slices > 1: kw.update(slices=slices, slices_plain=1)
    a = _sequence(GpuEncoder, O.default_config(w, h, **kw), frames, True)
    b = _sequence(GpuEncoder, O.default_config(w, h, **kw), frames, False)
    for (disp, mb_a, lv_a, rec_a), (_, mb_b, lv_b, rec_b) in zip(a, b):
        assert np.array_equal(mb_a.view(np.uint8), mb_b.view(np.uint8)), f"records of display picture {disp} differ"
        assert np.array_equal(lv_a, lv_b), f"levels of display picture {disp} differ"
        assert np.array_equal(rec_a, rec_b), f"reconstruction of display picture {disp} differs"
    # (the first issue was a different picture: the comparison is not vacuous)
    c = _sequence(GpuEncoder, O.default_config(w, h, **kw), frames, False, qp=30)
    assert not np.array_equal(c[2][3], a[2][3])


def _bucket(info, rate, size, init):
    fill, low = init * size, None
    for r, v in zip(info["recs"], info["vbv"]):
        fill -= 8 * (r[4] - int(v["filler"]))
        low = fill if low is None else min(low, fill)
        fill = min(fill + rate / 25.0, size)
    return low


def _device_and_checker(tmp_path, w, h, n, seed, scene, opts):
    """the session on the device (in process) and over the CPU checker (tests/stub, a child process)"""
    import host_lib as HL
    sys.path.insert(0, os.path.join(HERE, "stub"))
    import run_host_vbv
    from run_host_b import make_frames
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    info, stream, recon = run_host_vbv.session(HL, make_frames(w, h, n, seed, scene), w, h, dict(o.partition("=")[::2] if "=" in o else (o, None) for o in opts))
    out = str(tmp_path / "chk.h264")
    env = dict(os.environ)
    env.pop("X264GPU_BATCH", None)
    r = subprocess.run([sys.executable, os.path.join(HERE, "stub", "run_host_vbv.py"), out, str(w), str(h), str(n), str(seed), f"scene_len={scene}"] + opts,
                       capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-1500:]
    chk = json.loads(r.stdout.strip().splitlines()[-1])
    return info, stream, recon, chk, open(out, "rb").read()


@pytest.mark.parametrize("opts,bufsize", [
    (["crf=23", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=60"], 60),
    (["bitrate=100", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=60", "nal-hrd=cbr"], 60),
    (["bitrate=100", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=12", "nal-hrd=cbr"], 12),          # ... with filler
])
def test_vbv_session_equals_the_checker_session(gpu, tmp_path, opts, bufsize):
    """the 176x144 sessions of tests/test_vbv_cpu.py on the device: the same pictures, quantisers, re-encodes and bytes as the same host code over the CPU checker
    (lookahead costs, planned costs, coded sizes: everything the VBV reads comes from the device here), and the device's own stream holds the bucket"""
    info, stream, _, chk, chk_stream = _device_and_checker(tmp_path, 176, 144, 30, 3, 13, opts)
    assert [list(r) for r in info["recs"]] == chk["recs"]
    assert [int(v["attempts"]) for v in info["vbv"]] == [int(v["attempts"]) for v in chk["vbv"]]
    assert [v["planned"] for v in info["vbv"]] == [[tuple(x) for x in v["planned"]] for v in chk["vbv"]]
    assert stream == chk_stream
    assert _bucket(info, 100e3, bufsize * 1e3, 0.9) >= 0
    if bufsize == 12: assert any(v["filler"] for v in info["vbv"])


def test_guard_on_the_device(gpu, tmp_path):
    """64x48, no B pictures, 12 pictures with a scene cut at picture 6, crf 18 against vbv-maxrate 40 / vbv-bufsize 8 without lookahead.  Measured on the CPU
    checker: unconstrained, the pictures take 15 384 / 8 384 / 5 648 / 6 024 / 5 968 / 13 720 / 11 608 / ... bits (the scene cut: 13 720 > 8 000); at qp 51 every
    picture stays under the 1 600 bits a picture brings (120 .. 336 bits) except the first access unit, whose 1 712 bits include the parameter sets and fit the
    7 200 bits the buffer starts with — so the guard can always succeed.  The hook reports re-encodes, the bucket holds, the stream decodes to the reconstruction"""
    import oracle_lib as O
    opts = ["crf=18", "keyint=250", "bframes=0", "rc-lookahead=0", "vbv-maxrate=40", "vbv-bufsize=8"]
    info, stream, recon, chk, chk_stream = _device_and_checker(tmp_path, 64, 48, 12, 3, 6, opts)
    assert sum(int(v["attempts"]) - 1 for v in info["vbv"]) >= 1
    assert _bucket(info, 40e3, 8e3, 0.9) >= 0 and not any("VBV underflow" in m for _, m in info["log"])
    assert stream == chk_stream
    dec = O.h264_decode(stream, 12, 64, 48)
    assert len(dec) == 12 and np.array_equal(dec[-1], np.frombuffer(recon, np.uint8))

"""VBV rate control (--vbv-maxrate / --vbv-bufsize / --vbv-init, --nal-hrd) of the host encoder over the CPU stand-in device (tests/stub): the coded stream never
under-runs the buffer it was asked to respect, the rate control's numbers equal the Python twin's (tests/vbv_ref.py), the planned lists are x264's vbv_lookahead,
the HRD the stream signals holds when Annex C is replayed from the SEI values (tests/hrd_ref.py, a reader written from the specification), every stream decodes to
the session's reconstruction, the option rules of x264's validate_parameters give the stated effective parameters, and a session without VBV options writes the
bytes the commit before this feature wrote.

The clip: 176x144, 30 frames, synth seed 3 with a scene cut every 13 pictures, 25 fps.  Unconstrained (crf 23) it takes 34 827 bytes with I pictures of 5 750 /
6 713 / 5 216 bytes; at qp 51 its largest picture is 363 bytes and the whole stream 1 704.  Under vbv-maxrate 100 / vbv-bufsize 60 (start fill 0.9 x 60 000 bits,
4 000 bits a picture) the unconstrained stream under-runs at its third picture."""
import hashlib
import json
import os
import subprocess
import sys

import pytest

import hrd_ref
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
W, H, N, SEED, SCENE = 176, 144, 30, 3, 13
BASE = ["crf=23", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=60"]
SESSIONS = {
    "lookahead": BASE,
    "reactive": BASE + ["rc-lookahead=0"],
    "no_b": BASE + ["bframes=0", "weightp=0"],                                # the forced DPB-model route
    "abr": ["bitrate=80", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=20"],          # ABR below the VBV's rate (with 60 kbit of buffer the VBV never has to act at 80 kbit/s)
    "cbr": ["bitrate=100", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=60", "nal-hrd=cbr"],
    "vbr_hrd": BASE + ["nal-hrd=vbr"],
    # the 60 kbit buffer never fills within these 30 pictures (measured: it peaks at 32.8 kbit), so no filler is due there; three pictures' worth of buffer does fill
    "cbr_small": ["bitrate=100", "keyint=250", "rc-lookahead=10", "vbv-maxrate=100", "vbv-bufsize=12", "nal-hrd=cbr"],
}
QP51_BYTES = 1704
_cache = {}


def run(tmp, name, opts, w=W, h=H, n=N, seed=SEED, scene=SCENE, env=None):
    out = os.path.join(str(tmp), name + ".h264")
    e = dict(os.environ)
    e.pop("X264GPU_BATCH", None)
    e.update(env or {})
    r = subprocess.run([sys.executable, os.path.join(HERE, "stub", "run_host_vbv.py"), out, str(w), str(h), str(n), str(seed)] + ([f"scene_len={scene}"] if scene else []) + list(opts),
                       capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1]), open(out, "rb").read(), open(out + ".recon", "rb").read()


@pytest.fixture(scope="module")
def sessions(tmp_path_factory):
    """every session of SESSIONS, run once (about a second each on the stand-in)"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    tmp = tmp_path_factory.mktemp("vbv")

    def get(name):
        if name not in _cache:
            _cache[name] = run(tmp, name, SESSIONS[name])
        return _cache[name]
    return get


def bucket(info, maxrate_bits, bufsize_bits, init):
    """the leaky bucket of the issue: per access unit fill -= 8 (size - filler); fill >= 0; fill = min(fill + rate / fps, size).  -> the fills behind the removals"""
    fill, fills = init * bufsize_bits, []
    for (_, _, _, _, size), v in zip(info["recs"], info["vbv"]):
        fill -= 8 * (size - int(v["filler"]))
        fills.append(fill)
        fill = min(fill + maxrate_bits / 25.0, bufsize_bits)
    return fills


@pytest.mark.parametrize("name", ["lookahead", "reactive", "no_b", "abr", "cbr"])
def test_leaky_bucket_never_underruns(sessions, name):
    info, stream, _ = sessions(name)
    assert len(info["recs"]) == N and sum(r[4] for r in info["recs"]) == len(stream)
    bufsize = 20 if name == "abr" else 60
    assert (info["eff"]["vbv_maxrate"], info["eff"]["vbv_bufsize"]) == (100, bufsize) and abs(info["eff"]["vbv_init"] - 0.9) < 1e-6
    fills = bucket(info, 100e3, bufsize * 1e3, 0.9)
    print(name, len(stream), "bytes; lowest fill", min(fills), "attempts", [int(v["attempts"]) for v in info["vbv"]])
    assert min(fills) >= 0, (name, fills)
    assert not any("VBV underflow" in m for _, m in info["log"])
    assert len(stream) > 4 * QP51_BYTES, "the session must not simply run at qp_max"
    acted = [v for r, v in zip(info["recs"], info["vbv"]) if v["attempts"] > 1 or (r[0] <= 3 and v["qp_novbv"] != v["qp_clipped"])]
    assert acted, "neither a re-encode nor a clipped quantiser: the VBV did nothing"
    # the rate control's own account is the bucket's (it starts a picture less the header NAL units, and is no fuller than the nominal bucket)
    for v, f in zip(info["vbv"], fills):
        assert v["fill_after"] - v["max_rate"] / 25.0 <= f + 1e-6 or v["fill_after"] == v["buffer_size"]


def test_unconstrained_stream_underruns(sessions, tmp_path):
    """what the bucket test is worth: the same clip without VBV options breaks it at its third picture"""
    info, stream, _ = run(tmp_path, "free", ["crf=23", "keyint=250", "rc-lookahead=10"])
    assert len(stream) == 34827 and info["vbv"][0] is None
    fill, bad = 0.9 * 60e3, []
    for k, r in enumerate(info["recs"]):
        fill -= 8 * r[4]
        if fill < 0: bad.append(k)
        fill = min(max(fill, 0) + 4000, 60e3)
    assert bad and bad[0] == 2


def test_guard_reencodes_and_reports(sessions):
    info, _, _ = sessions("reactive")
    again = [(r, v, d) for r, v, d in zip(info["recs"], info["vbv"], info["decisions"]) if v["attempts"] > 1]
    assert again, "the reactive session on this clip re-encodes its first picture"
    for r, v, d in again:
        # what is reported describes the attempt that was emitted: the integer quantiser, the float one equal to it, a size that fits what start() saw
        assert v["qp_final"] == d[0] and d[3] == float(d[0]) and v["qp_final"] > round(v["qp_clipped"])
        assert 8 * r[4] - v["overhead_bits"] <= v["fill_before"] or d[0] == info["eff"]["qp_max"]
    assert sum(1 for lvl, m in info["log"] if lvl == 3 and "coded again" in m) == sum(int(v["attempts"]) - 1 for v in info["vbv"])


@pytest.mark.parametrize("name", ["lookahead", "no_b", "cbr"])
def test_planned_lists(sessions, name):
    """x264's vbv_lookahead: every I / P picture carries the types and costs of the pictures coded after it, in coding order, closed by AUTO"""
    info, _, _ = sessions(name)
    recs, vbv = info["recs"], info["vbv"]
    cls = {1: "I", 2: "I", 3: "P", 4: "B", 5: "B"}          # X264_TYPE_IDR, I, P, BREF, B
    pcls = {0: "I", 1: "I", 2: "P", 3: "B", 4: "B"}         # PIC_IDR, I, P, BREF, B
    actual = [cls[r[0]] for r in recs]
    checked = full = 0
    for k, (r, v) in enumerate(zip(recs, vbv)):
        if actual[k] == "B":
            assert v["planned"] == [] and v["planned_end"] == -1
            continue
        assert v["planned_end"] == -1, "the list of a non-B picture ends in AUTO"
        plan = [pcls[t] for t, _ in v["planned"]]
        assert all(c > 0 for _, c in v["planned"])
        assert len(plan) <= info["eff"]["lookahead"] + info["eff"]["bframes"] + 1
        # its first entries are the B pictures of its own mini-GOP (coded right behind it), then the next non-B picture
        nb = 0
        while k + 1 + nb < N and actual[k + 1 + nb] == "B": nb += 1
        if plan:
            assert plan[:nb] == ["B"] * nb, (k, plan, actual[k + 1:])
            checked += 1
        # ... and the plan is what is coded, up to the first picture that was decided again later (a scene cut found once it came into reach, b-adapt with more to see)
        m = 0
        while m < len(plan) and k + 1 + m < N and plan[m] == actual[k + 1 + m]: m += 1
        assert m >= min(nb, len(plan))
        if m == len(plan) or k + 1 + m == N: full += 1
        elif name == "no_b": assert plan[m] == "P" and actual[k + 1 + m] == "I", "without B pictures only a scene cut changes a planned type"
    assert checked >= 8 and full >= 4, (checked, full)
    assert vbv[0]["planned"], "the first keyframe has a plan too (the analysis runs again behind a keyframe)"


@pytest.mark.parametrize("name", ["vbr_hrd", "cbr", "cbr_small"])
def test_hrd_syntax_and_annex_c(sessions, name):
    info, stream, _ = sessions(name)
    cbr = name != "vbr_hrd"
    assert info["eff"]["nal_hrd"] == (2 if cbr else 1)
    sps, aus = hrd_ref.access_units(stream)
    hrd = sps["vui"]["nal_hrd"]
    assert hrd is not None and sps["vui"]["vcl_hrd"] is None and sps["vui"]["low_delay_hrd_flag"] == 0 and sps["vui"]["pic_struct_present"] == 0
    assert hrd["cpb_cnt"] == 1 and hrd["time_offset_length"] == 0 and hrd["sched"][0]["cbr_flag"] == int(cbr)
    rate, size = hrd["sched"][0]["bit_rate"], hrd["sched"][0]["cpb_size"]
    # value << scale keeps the request up to the low bits the notation drops; the rate control runs on exactly what is signalled
    assert 0 <= 100000 - rate < 64 << hrd["bit_rate_scale"] and 0 <= info["eff"]["vbv_bufsize"] * 1000 - size < 16 << hrd["cpb_size_scale"]
    assert all(v["max_rate"] == rate and v["buffer_size"] == size for v in info["vbv"])
    assert len(aus) == N and [a["bytes"] for a in aus] == [r[4] for r in info["recs"]]
    assert [a["filler"] for a in aus] == [int(v["filler"]) for v in info["vbv"]]
    for a, r in zip(aus, info["recs"]):
        assert (a["bp"] is not None) == bool(r[3]), "a buffering period in front of every keyframe, and nowhere else"
        assert a["pt"] is not None
    # the delays say what the buffer held: floor(90000 fill / rate), complemented to the buffer's size
    first = info["vbv"][0]
    fill0 = first["fill_before"] + first["overhead_bits"]
    assert aus[0]["bp"]["initial_cpb_removal_delay"][0] == int(90000 * fill0 / rate)
    for a in aus:
        if a["bp"]: assert sum(a["bp"]["initial_cpb_removal_delay"] + a["bp"]["initial_cpb_removal_delay_offset"]) == int(90000 * size / rate)
    rp = hrd_ref.replay(sps, aus)
    tc = hrd_ref.Fraction(sps["vui"]["num_units_in_tick"], sps["vui"]["time_scale"])
    for k, t in enumerate(rp):
        assert t["t_af"] <= t["t_r"], f"access unit {k} has not arrived when it is removed: {float(t['t_af'])} > {float(t['t_r'])}"
        if k: assert t["t_r"] - rp[k - 1]["t_r"] == 2 * tc
    by_display = sorted(range(N), key=lambda k: info["recs"][k][1])
    outs = [rp[k]["t_o"] for k in by_display]
    assert all(b - a == 2 * tc for a, b in zip(outs, outs[1:])), "output times: display order, two ticks apart"
    assert all(t["t_o"] >= t["t_r"] for t in rp)
    if cbr:
        total_bits = 8 * len(stream)
        assert total_bits >= N * rate / 25.0 - size
        fills = bucket(info, rate, size, info["eff"]["vbv_init"])
        # the bucket with the filler IN the stream never holds more than its size: arrival at the signalled rate never has to stop
        fill = info["eff"]["vbv_init"] * size
        for r in info["recs"]:
            fill = fill - 8 * r[4] + rate / 25.0
            assert fill <= size + 1e-6
        assert min(fills) >= 0
    if name == "cbr_small":
        assert any(a["filler"] for a in aus) and any(12 in t for t in info["nal_types"]), "filler NAL units expected"
    if os.path.exists(O.LSMASH_REF):
        lsps, _, sl = O.lsmash_parse(stream)
        assert len(sl) == N and (lsps.cropped_width, lsps.cropped_height) == (W, H) and (lsps.num_units_in_tick, lsps.time_scale) == (1, 50)
        assert [s.nal_unit_type for s in sl] == [5 if r[3] else 1 for r in info["recs"]]


@pytest.mark.parametrize("name", sorted(SESSIONS))
def test_stream_decodes_to_the_reconstruction(sessions, name):
    """closed loop: pictures that were coded again leave the DPB as the decoder has it"""
    import numpy as np
    info, stream, recon = sessions(name)
    dec = O.h264_decode(stream, N, W, H)
    assert len(dec) == N
    assert np.array_equal(dec[-1], np.frombuffer(recon, np.uint8)), "the last coded picture's reconstruction differs from the decoder's"


MATRIX = [
    # options, effective (maxrate, bufsize, nal_hrd[, bitrate]), a piece of the log line
    (["qp=30", "vbv-maxrate=100", "vbv-bufsize=60"], (0, 0, 0), "VBV is incompatible with constant QP"),
    (["bitrate=100", "vbv-bufsize=60"], (100, 60, 0), "assuming CBR"),
    (["crf=23", "vbv-bufsize=60"], (0, 0, 0), "bufsize set but maxrate unspecified, ignored"),
    (["crf=23", "vbv-maxrate=100"], (0, 0, 0), "maxrate specified, but no bufsize, ignored"),
    (["bitrate=200", "vbv-maxrate=100", "vbv-bufsize=60"], (100, 60, 0, 100), "max bitrate less than average bitrate"),
    (["crf=23", "vbv-maxrate=100", "vbv-bufsize=2"], (100, 4, 0), "cannot be smaller than one frame"),
    (["crf=23", "nal-hrd=vbr"], (0, 0, 0), "NAL HRD parameters require VBV parameters"),
    (["crf=23", "vbv-maxrate=100", "vbv-bufsize=60", "nal-hrd=cbr"], (100, 60, 1), "CBR HRD requires constant bitrate"),
    (["bitrate=80", "vbv-maxrate=100", "vbv-bufsize=60", "nal-hrd=cbr"], (100, 60, 1), "CBR HRD requires constant bitrate"),
    (["bitrate=100", "vbv-maxrate=100", "vbv-bufsize=60", "nal-hrd=cbr"], (100, 60, 2), "VBV: maxrate"),
    (["crf=23", "vbv-maxrate=100", "vbv-bufsize=60", "threads=2", "keyint=4"], (0, 0, 0), "needs %s"),
]


@pytest.mark.parametrize("opts,want,needle", MATRIX)
def test_validation_matrix(tmp_path, opts, want, needle):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    info, _, _ = run(tmp_path, "m", opts, 64, 48, 3, 5, 0)
    eff = info["eff"]
    assert (eff["vbv_maxrate"], eff["vbv_bufsize"], eff["nal_hrd"]) == want[:3], eff
    if len(want) > 3: assert eff["bitrate"] == want[3]
    assert any(needle in m for lvl, m in info["log"] if lvl <= 2), [m for _, m in info["log"]]
    if want[0]:          # VBV runs: the open line says what it runs with, and the session is serial on the DPB model
        line = [m for lvl, m in info["log"] if lvl == 2 and m.startswith("VBV:")]
        assert line and "maxrate" in line[0] and "bufsize" in line[0] and "init" in line[0] and "picture re-encode" in line[0]
        assert all(v is not None for v in info["vbv"])
    else:
        assert all(v is None for v in info["vbv"])


def test_vbv_init_rules(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    base = ["crf=23", "vbv-maxrate=100", "vbv-bufsize=60"]
    for init, want in (("30", 0.5), ("0.01", 4.0 / 60.0), ("0.5", 0.5), ("500", 1.0)):          # above 1: kbit; never below one picture's arrival, never above 1
        info, _, _ = run(tmp_path, "i", base + [f"vbv-init={init}"], 64, 48, 2, 5, 0)
        assert abs(info["eff"]["vbv_init"] - want) < 1e-6, (init, info["eff"]["vbv_init"])
        assert abs(info["vbv"][0]["fill_before"] + info["vbv"][0]["overhead_bits"] - want * 60e3) < 0.01


def test_refused_under_batch_and_in_a_second_pass(tmp_path):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    vbv = ["vbv-maxrate=100", "vbv-bufsize=60"]
    # (scenecut stays on, so the session does not wait for a partner: it runs on its own — and without VBV)
    info, _, _ = run(tmp_path, "b", ["crf=23"] + vbv, 64, 48, 3, 5, 0, env={"X264GPU_BATCH": "2"})
    assert info["eff"]["vbv_maxrate"] == 0 and any("X264GPU_BATCH" in m or "needs %s" in m for lvl, m in info["log"] if lvl <= 1)
    st = str(tmp_path / "p.stats")
    run(tmp_path, "p1", ["bitrate=100", "pass=1", f"stats={st}"], 64, 48, 6, 5, 0)
    info, _, _ = run(tmp_path, "p2", ["bitrate=100", "pass=2", f"stats={st}"] + vbv, 64, 48, 6, 5, 0)
    assert info["eff"]["vbv_maxrate"] == 0 and all(v is None for v in info["vbv"])
    assert any("needs %s" in m for lvl, m in info["log"] if lvl <= 1)


def test_sessions_without_vbv_are_byte_identical_to_the_parent(tmp_path):
    """tests/golden/vbv_parent_streams.json: size, SHA-256, picture types and sizes of four sessions on the clip, recorded with the stand-in build of the commit before
    this feature"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    gold = json.load(open(os.path.join(HERE, "golden", "vbv_parent_streams.json")))
    assert len(gold) == 4
    for name, g in gold.items():
        info, stream, _ = run(tmp_path, name, g["opts"])
        assert [r[4] for r in info["recs"]] == g["sizes"] and [r[0] for r in info["recs"]] == g["types"], name
        assert len(stream) == g["bytes"] and hashlib.sha256(stream).hexdigest() == g["sha256"], name
        assert all(v is None for v in info["vbv"])


@pytest.mark.parametrize("name", ["lookahead", "abr", "cbr", "reactive", "no_b", "cbr_small"])
def test_rate_control_equals_the_twin(sessions, name):
    """tests/vbv_ref.py fed what the session saw (types, lookahead costs, planned lists, header bits, coded sizes, the quantisers pictures were finally coded with)
    computes the same float quantisers, planned sizes and buffer fills: to a part in 10^9, the bar tests/test_decisions_cpu.py sets for the same double arithmetic
    restated in another language; integer quantisers exactly"""
    import vbv_ref
    info, _, _ = sessions(name)
    twin = vbv_ref.replay(info, (W + 15) // 16, (H + 15) // 16)

    def close(a, b):
        return abs(a - b) <= 1e-9 * max(abs(a), abs(b), 1e-300)
    for k, (t, v, d, r) in enumerate(zip(twin, info["vbv"], info["decisions"], info["recs"])):
        tag = (name, k, r[0])
        assert close(t["fill_before"], v["fill_before"]), (tag, t["fill_before"], v["fill_before"])
        assert close(t["frame_size_planned"], v["frame_size_planned"]), (tag, t["frame_size_planned"], v["frame_size_planned"])
        if t["qp"] is not None:
            assert close(t["qp_novbv"], v["qp_novbv"]), (tag, t["qp_novbv"], v["qp_novbv"])
            assert close(t["qp_clipped"], v["qp_clipped"]), (tag, t["qp_clipped"], v["qp_clipped"])
            if v["attempts"] == 1: assert t["qp"] == d[0], (tag, t["qp"], d[0])
        assert close(t["fill_after"], v["fill_after"]), (tag, t["fill_after"], v["fill_after"])
        assert t["filler"] == int(v["filler"]), tag


_MP4_SCRIPT = r"""
import ctypes as C, os, sys
os.environ["X264_HOST_STUB"] = "1"
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import host_lib as V
D = V.H.DriverProc
ico = V.ICOPEN(fccType=V.fourcc(b"vidc"))
cid = D(0, None, V.DRV_OPEN, 0, V.addr(ico))
n = D(cid, None, V.ICM_GETSTATE, 0, 0)
cfg = V.VfwConfig()
D(cid, None, V.ICM_GETSTATE, V.addr(cfg), n)
cfg.i_log_level = 3
cfg.extra_cmdline = sys.argv[2].encode()
assert D(cid, None, V.ICM_SETSTATE, V.addr(cfg), n) == n
inb, outb = V.bmi(64, 48, b"I420"), V.BITMAPINFO()
D(cid, None, V.ICM_COMPRESS_GET_FORMAT, V.addr(inb), V.addr(outb))
assert D(cid, None, V.ICM_COMPRESS_BEGIN, V.addr(inb), V.addr(outb)) == V.ICERR_OK
print(V.H.x264vfw_shim_log(cid).decode())
D(cid, None, V.ICM_COMPRESS_END, 0, 0)
D(cid, None, V.DRV_CLOSE, 0, 0)
"""


@pytest.mark.parametrize("ext,hrd", [("mp4", "nal-hrd vbr"), ("mkv", "nal-hrd cbr")])
def test_driver_turns_cbr_hrd_into_vbr_for_mp4(tmp_path, ext, hrd):
    """codec.c:1126-1129: mp4 carries no filler, so the driver opens the encoder with a VBR HRD there (and says so); other containers keep cbr"""
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    cmdline = f"--output {tmp_path}/t.{ext} --bitrate 100 --vbv-maxrate 100 --vbv-bufsize 60 --nal-hrd cbr"
    r = subprocess.run([sys.executable, "-c", _MP4_SCRIPT, HERE, cmdline], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-1500:]
    assert ("cbr nal-hrd is not compatible with mp4" in r.stdout) == (ext == "mp4")
    assert hrd in r.stdout

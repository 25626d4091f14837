"""The sessions of the macroblock-tree statistics tests (tests/test_mbtree_stats_cpu.py over the CPU stand-in, tests/test_gpu_mbtree_stats.py on the device): one
clip, the options the issue names, every session a child process (tests/stub/run_host_mbtree.py), and the assertions both files make of a first and a second pass."""
import hashlib
import json
import os
import subprocess
import sys

import numpy as np

import mbtree_stats_ref as R
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(os.path.dirname(HERE), "oracle"))
import decide as D  # noqa: E402

SEED, SCENE, NFR = 3, 7, 20          # (chosen on the CPU: the clip has I, P, B-reference and b pictures, and the tree moves the offsets of every kept picture)
TOOLS = ["bframes=3", "b-pyramid=normal", "keyint=12", "rc-lookahead=8", "subme=5", "trellis=0", f"scene_len={SCENE}"]
TODAY = "2-pass: the macroblock-tree statistics file is not implemented in the MI355X path: mbtree 0 in both passes"
X264_TYPE = {1: "I", 2: "i", 3: "P", 4: "B", 5: "b"}          # pic_out->i_type -> the statistics' character


def nmb_of(w, h):
    return ((w + 15) // 16) * ((h + 15) // 16)


def frames_of(w, h):
    from synth import synth_frames
    return synth_frames(w, h, NFR, seed=SEED, scene_len=SCENE)


def run_many(sessions, opt_in, device=False):
    """sessions: [(out, w, h, opts, hook)], run one after the other in ONE child process -> [(info, stream bytes, [offsets of every output picture: float32 array or None])]"""
    if not device:
        subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    env = {k: v for k, v in os.environ.items() if k != "X264GPU_MBTREE_STATS"}
    if opt_in:
        env["X264GPU_MBTREE_STATS"] = "1"
    cmd = [sys.executable, os.path.join(HERE, "stub", "run_host_mbtree.py")]
    for i, (out, w, h, opts, hook) in enumerate(sessions):
        cmd += (["--"] if i else []) + [str(out), str(w), str(h), str(NFR), str(SEED)] + TOOLS + list(opts) + (["hook=1"] if hook else []) + (["device=1"] if device else [])
    r = subprocess.run(cmd, capture_output=True, text=True, timeout=600, env=env)
    assert r.returncode == 0, r.stderr[-3000:]
    infos = [json.loads(ln) for ln in r.stdout.strip().splitlines() if ln.startswith("{")]
    assert len(infos) == len(sessions)
    return [_collect(info, out, w, h, hook) for info, (out, w, h, _o, hook) in zip(infos, sessions)]


def run(out, w, h, opts, opt_in, device=False, hook=True):
    return run_many([(out, w, h, opts, hook)], opt_in, device)[0]


def _collect(info, out, w, h, hook):
    offs = []
    if hook and info.get("opened"):
        nmb, raw = nmb_of(w, h), open(str(out) + ".offsets", "rb").read()
        for k in range(len(raw) // (1 + 4 * nmb)):
            rec = raw[k * (1 + 4 * nmb):(k + 1) * (1 + 4 * nmb)]
            offs.append(np.frombuffer(rec[1:], np.float32).copy() if rec[0] else None)
    return info, (open(out, "rb").read() if info.get("opened") else b""), offs


def texts(info, level=None):
    return [t for lvl, _fmt, t in info["log"] if level is None or lvl == level]


def stat_lines(path):
    return open(path).read().splitlines()


def sha(b):
    return hashlib.sha256(b).hexdigest()


def check_first_pass(w, h, stats, info, stream, offs, plain_stream, path_word):
    """the assertions of a first pass that writes the tree file (issue: CPU test 3 / GPU test 2); -> the records"""
    nmb = nmb_of(w, h)
    assert info["mbtree"] == 1 and info["rc_lookahead"] == 8 and info["failed_at"] is None
    assert any(f"packed on the {path_word}" in t for t in texts(info, 2)), texts(info)
    lines = stat_lines(stats)
    assert lines[0].startswith(f"#options: {w}x{h} ") and lines[0].endswith(" mbtree=1 rc_lookahead=8"), lines[0]
    kept = R.kept_lines(lines)
    tree = str(stats) + ".mbtree"
    assert os.path.getsize(tree) == len(kept) * (1 + 2 * nmb) and not os.path.exists(tree + ".temp")
    recs = R.read_file(tree, nmb)
    assert [t for t, _ in recs] == [R.TYPE_OF_CHAR[c] for _, _, c in kept]
    types = [X264_TYPE[r[0]] for r in info["recs"]]
    assert {"I", "P", "B", "b"} <= set(types), types          # every kind of picture is in the clip
    assert [c for _, _, c in kept] == [t for t in types if t != "b"]
    # every record is the pack of what its picture was coded with; b pictures are coded with their AQ offsets and have no record
    strength = float(np.float32(info["aq_strength"]) * np.float32(1.0397))
    frames = frames_of(w, h)
    moved = 0
    for (out, disp, _c), (_t, words) in zip(kept, recs):
        assert offs[out] is not None and np.array_equal(R.pack(offs[out]), words), f"record of coded picture {out}"
        moved += not np.array_equal(R.pack(O.aq_offsets(frames[disp], w, h, strength)), words)
    assert moved >= 1, "the tree moved nothing: every record is the pack of the AQ offsets"
    for k, r in enumerate(info["recs"]):
        if X264_TYPE[r[0]] == "b":
            assert np.array_equal(offs[k], O.aq_offsets(frames[r[1]], w, h, strength)), f"b picture {k}: not the AQ offsets alone"
    assert stream == plain_stream, "the first pass' stream differs from the same session without pass=1"
    return recs


def check_second_pass(w, h, stats, kbps, info, stream, offs, first_info, first_offs, path_word):
    """the assertions of a second pass over the tree file (issue: CPU test 4 / GPU test 3)"""
    nmb = nmb_of(w, h)
    assert info["mbtree"] == 1 and info["rc_lookahead"] == 0 and info["failed_at"] is None
    assert any(f"unpacked on the {path_word}" in t for t in texts(info, 2)), texts(info)
    assert not any(lvl <= 1 for lvl, _f, _t in info["log"]), texts(info)
    lines = stat_lines(stats)
    # types follow the statistics, in coding order
    by_out = sorted((int(dict(x.split(":", 1) for x in ln.split() if ":" in x)["out"]), ln) for ln in lines if not ln.startswith("#"))
    want_types = [dict(x.split(":", 1) for x in ln.split() if ":" in x)["type"] for _, ln in by_out]
    assert [X264_TYPE[r[0]] for r in info["recs"]] == want_types
    assert [r[1] for r in info["recs"]] == [r[1] for r in first_info["recs"]]
    recs = R.read_file(str(stats) + ".mbtree", nmb)
    k = 0
    for out, t in enumerate(want_types):
        if t == "b":
            assert np.array_equal(offs[out], first_offs[out]), f"b picture {out}: not the first pass' AQ offsets"
        else:
            assert np.array_equal(offs[out], R.unpack(recs[k][1])), f"kept picture {out}: not unpack(record {k})"
            k += 1
    assert k == len(recs)
    # the plan and the feedback on top of it
    E = R.init_pass2_tree(lines, nmb, kbps)
    plan = info["plan"]
    assert plan["count"] == NFR
    got_q, want_q = np.array(plan["new_qscale"]), np.array([e.new_qscale for e in E])
    assert np.allclose(got_q, want_q, rtol=1e-9, atol=0), np.abs(got_q / want_q - 1).max()
    got_b, want_b = np.array(plan["expected_bits"]), np.array([e.expected_bits for e in E])
    assert np.allclose(got_b, want_b, rtol=1e-9, atol=1e-6), np.abs(got_b - want_b).max()
    fb = D.pass2_quantisers(E, [r[4] for r in info["recs"]], kbps)
    assert [r[1] for r in info["recs"]] == [f for f, _, _ in fb]
    for j, ((f, qp, qpf), (gqp, gqpm)) in enumerate(zip(fb, info["qpm"])):
        assert gqp == qp and np.float32(gqpm) == np.float32(qpf), (kbps, j, f, gqp, gqpm, qp, qpf)
    assert len(O.h264_decode(stream, NFR, w, h)) == NFR

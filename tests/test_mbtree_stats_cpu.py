"""The macroblock-tree statistics file of 2-pass encodes (x264's <stats>.mbtree; host/mbtreestats.cpp, X264GPU_MBTREE_STATS=1) through the host library over the
CPU stand-in: the number format's known answers, the twin of the second pass' plan against the oracle's, a first pass that writes the file, a second pass and an
N-th pass that read it, every fallback, and the sessions without the variable against what the commit before produced."""
import json
import os
import re
import shutil

import numpy as np
import pytest

import mbtree_sessions as S
import mbtree_stats_ref as R
import oracle_lib as O

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
D = S.D
W, H, KBPS = 176, 144, (200, 90)


# ---- 1: the twin's number format ----
def test_pack_known_answers():
    x = [0.0, -0.0, 1 / 256, -1 / 256, 0.999 / 256, -0.999 / 256, 1.5, -1.5, 127.99609375, 200.0, -200.0, float("nan")]
    want = [0, 0, 1, -1, 0, 0, 384, -384, 0x7FFF, 0x7FFF, -0x8000, 0]
    got = R.pack(x)
    assert got.astype(np.int32).tolist() == want
    # byte order on the wire: the high byte first
    assert got.tobytes() == b"".join(int(v & 0xFFFF).to_bytes(2, "big") for v in want)
    assert R.pack([1.5]).tobytes() == b"\x01\x80" and R.pack([-200.0]).tobytes() == b"\x80\x00"
    assert R.unpack(b"\x01\x80")[0] == np.float32(1.5) and R.unpack(b"\xff\xff")[0] == np.float32(-1 / 256)


def test_pack_round_trip():
    x = np.random.default_rng(5).uniform(-127.9, 127.9, 4096).astype(np.float32)
    y = R.unpack(R.pack(x))
    assert np.all(np.abs(y - x) < 1 / 256) and np.all(np.abs(y) <= np.abs(x))          # within a step, never further from zero
    w = np.arange(-32768, 32768).astype(">i2")
    assert np.array_equal(R.pack(R.unpack(w)), w)


# ---- the sessions of the 176x144 clip, run once ----
class World:
    pass


@pytest.fixture(scope="module")
def world(tmp_path_factory):
    d = tmp_path_factory.mktemp("mbtree")
    wd = World()
    wd.dir, wd.stats = d, d / "x264.stats"
    st = [f"stats={wd.stats}"]
    wd.p1 = S.run(d / "p1.h264", W, H, st + ["crf=24", "pass=1"], True)
    wd.plain = S.run(d / "plain.h264", W, H, ["crf=24"], True, hook=False)
    wd.first_stats = wd.stats.read_bytes()
    wd.tree_bytes = (d / "x264.stats.mbtree").read_bytes()
    # today's second pass over the same statistics (no variable)
    wd.p2_plain = S.run(d / "p2_plain.h264", W, H, st + [f"bitrate={KBPS[0]}", "pass=2"], False)
    return wd


# ---- 2: the twin is a yardstick ----
def test_twin_plan_without_the_tree_equals_the_oracle(world, tmp_path):
    """init_pass2_tree with the tree switched off against oracle/decide.py init_pass2, over a statistics file a host session wrote"""
    st = tmp_path / "plain.stats"
    S.run(tmp_path / "a.h264", W, H, [f"stats={st}", "bitrate=200", "pass=1"], False, hook=False)
    lines = S.stat_lines(st)
    assert not lines[0].endswith("rc_lookahead=8")
    for kbps in KBPS:
        a, b = R.init_pass2_tree(lines, S.nmb_of(W, H), kbps, tree=False), D.init_pass2(lines, S.nmb_of(W, H), kbps)
        assert np.allclose([e.new_qscale for e in a], [e.new_qscale for e in b], rtol=1e-12, atol=0)
        assert np.allclose([e.expected_bits for e in a], [e.expected_bits for e in b], rtol=1e-12, atol=0)
        assert len({round(e.new_qscale, 6) for e in a}) > 3


# ---- 3: the first pass ----
def test_first_pass_writes_the_tree_file(world):
    info, stream, offs = world.p1
    S.check_first_pass(W, H, world.stats, info, stream, offs, world.plain[1], "host")


def test_first_pass_writes_the_tree_file_12_macroblocks(tmp_path):
    w, h = 64, 48
    st = tmp_path / "s.stats"
    info, stream, offs = S.run(tmp_path / "p1.h264", w, h, [f"stats={st}", "crf=24", "pass=1"], True)
    _i, plain, _o = S.run(tmp_path / "plain.h264", w, h, ["crf=24"], True, hook=False)
    S.check_first_pass(w, h, st, info, stream, offs, plain, "host")


# ---- 4: the second pass ----
@pytest.mark.parametrize("kbps", KBPS)
def test_second_pass_reads_the_tree_file(world, tmp_path, kbps):
    info, stream, offs = S.run(tmp_path / "p2.h264", W, H, [f"stats={world.stats}", f"bitrate={kbps}", "pass=2", "plan=1"], True)
    S.check_second_pass(W, H, world.stats, kbps, info, stream, offs, world.p1[0], world.p1[2], "host")
    if kbps == KBPS[0]:
        assert world.p2_plain[0]["mbtree"] == 0 and stream != world.p2_plain[1]          # the tree changes the second pass
    assert world.stats.read_bytes() == world.first_stats and (world.dir / "x264.stats.mbtree").read_bytes() == world.tree_bytes


# ---- 5: the N-th pass ----
def test_nth_pass_reads_and_keeps_the_tree_file(world, tmp_path):
    st = tmp_path / "x264.stats"
    shutil.copy(world.stats, st)
    shutil.copy(str(world.stats) + ".mbtree", str(st) + ".mbtree")
    info, stream, _o = S.run(tmp_path / "p3.h264", W, H, [f"stats={st}", f"bitrate={KBPS[0]}", "pass=3"], True)          # statistics read and written again
    assert info["mbtree"] == 1 and info["stat_read"] and info["stat_write"] and info["failed_at"] is None
    assert (tmp_path / "x264.stats.mbtree").read_bytes() == world.tree_bytes
    assert sorted(os.listdir(tmp_path)) == ["p3.h264", "p3.h264.offsets", "x264.stats", "x264.stats.mbtree"]          # no .temp of either file is left
    lines = S.stat_lines(st)
    assert len([ln for ln in lines if not ln.startswith("#")]) == S.NFR and st.read_bytes() != world.first_stats          # the statistics were written again


# ---- 6: the fallbacks ----
def _break_header(d, st):
    text = open(st).read()
    open(st, "w").write(text.replace(" mbtree=1 rc_lookahead=8", "", 1))


def _remove_file(d, st):
    os.remove(str(st) + ".mbtree")


def _truncate(d, st):
    raw = open(str(st) + ".mbtree", "rb").read()
    open(str(st) + ".mbtree", "wb").write(raw[:-1])


def _other_resolution(d, st):
    text = open(st).read()
    open(st, "w").write(text.replace(f"#options: {W}x{H} ", f"#options: {W + 16}x{H} ", 1))


@pytest.mark.parametrize("damage,word", [(_break_header, "header lacks mbtree=1"), (_remove_file, "missing"), (_truncate, "truncated"), (_other_resolution, "resolution changed")])
def test_fallbacks_run_the_tree_less_second_pass(world, tmp_path, damage, word):
    st = tmp_path / "x264.stats"
    shutil.copy(world.stats, st)
    shutil.copy(str(world.stats) + ".mbtree", str(st) + ".mbtree")
    damage(tmp_path, st)
    info, stream, _o = S.run(tmp_path / "p2.h264", W, H, [f"stats={st}", f"bitrate={KBPS[0]}", "pass=2"], True)
    warnings = S.texts(info, 1)
    assert len(warnings) == 1 and word in warnings[0] and warnings[0].endswith("mbtree 0"), S.texts(info)
    assert info["mbtree"] == 0 and info["failed_at"] is None
    assert stream == world.p2_plain[1]          # today's tree-less second pass, byte for byte


# ---- 7: a record of another picture type ----
def test_flipped_type_byte_fails_the_encode(world, tmp_path):
    st = tmp_path / "x264.stats"
    shutil.copy(world.stats, st)
    raw = bytearray(world.tree_bytes)
    rs = R.record_size(S.nmb_of(W, H))
    assert raw[2 * rs] == R.SLICE_TYPE_P
    raw[2 * rs] = R.SLICE_TYPE_B          # the third kept picture
    open(str(st) + ".mbtree", "wb").write(bytes(raw))
    info, _stream, _o = S.run(tmp_path / "p2.h264", W, H, [f"stats={st}", f"bitrate={KBPS[0]}", "pass=2"], True)
    assert info["failed_at"] is not None and len(info["recs"]) == 2
    errors = [(f, t) for lvl, f, t in info["log"] if lvl == 0]
    assert ("MB-tree frametype %d doesn't match actual frametype %d.", "MB-tree frametype 1 doesn't match actual frametype 0.") in errors, errors


# ---- 8: without the variable ----
def test_without_the_variable_both_passes_are_the_parents(tmp_path):
    g = json.load(open(os.path.join(HERE, "golden", "mbtree_stats_parent.json")))
    st = tmp_path / "x264.stats"
    opts = [f"stats={st}", f"bitrate={g['bitrate']}"]
    i1, s1, _o = S.run(tmp_path / "p1.h264", g["width"], g["height"], opts + ["pass=1"], False)
    first = st.read_bytes()
    i2, s2, _o = S.run(tmp_path / "p2.h264", g["width"], g["height"], opts + ["pass=2"], False)
    for info in (i1, i2):
        assert info["mbtree"] == 0 and S.TODAY in S.texts(info, 2), S.texts(info)
        assert not any("statistics file, " in t for t in S.texts(info))
    assert not [f for f in os.listdir(tmp_path) if "mbtree" in f]
    assert not first.splitlines()[0].endswith(b"rc_lookahead=8") and b"mbtree" not in first
    assert (S.sha(s1), S.sha(first), S.sha(s2)) == (g["first_pass_stream"], g["first_pass_stats"], g["second_pass_stream"])


# ---- 9: the new entries are in the header, the binding and the library ----
def test_exports():
    import subprocess
    dev_h = open(os.path.join(ROOT, "include", "x264gpu.h")).read()
    host_h = open(os.path.join(ROOT, "include", "x264gpu_host.h")).read()
    assert re.search(r"int\s+x264gpu_mbtree_pack\s*\(const float \*d_offsets, int n, uint16_t \*d_out, void \*stream\);", dev_h)
    assert re.search(r"int\s+x264gpu_mbtree_unpack\s*\(const uint16_t \*d_in, int n, float \*d_offsets, void \*stream\);", dev_h)
    assert "int x264host_last_mb_qp_offsets(x264_t *h, float *dst, int n);" in host_h
    lib_py = open(os.path.join(ROOT, "x264vfw_amd", "lib.py")).read()
    api_py = open(os.path.join(ROOT, "x264vfw_amd", "host_api.py")).read()
    assert '"x264gpu_mbtree_pack"' in lib_py and '"x264gpu_mbtree_unpack"' in lib_py and '"x264host_last_mb_qp_offsets"' in api_py
    # the device unit defines the two entries; the host library (here: the one over the CPU stand-in, which has no device entries) exports the hook and
    # binds the device entries weakly
    unit = open(os.path.join(ROOT, "x264vfw_amd", "csrc", "mbtree_stats.hip")).read()
    assert "int x264gpu_mbtree_pack(" in unit and "int x264gpu_mbtree_unpack(" in unit
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    nm = subprocess.run(["nm", "-D", os.path.join(HERE, "stub", "_build", "libx264gpu_host.so")], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT x264host_last_mb_qp_offsets\b", nm)
    assert re.search(r"\bw x264gpu_mbtree_pack\b", nm) and re.search(r"\bw x264gpu_mbtree_unpack\b", nm)
    for so in (os.path.join(ROOT, "x264vfw_amd", "libx264gpu.so"),):
        if os.path.exists(so):          # (a tree that has been built: the product's device library)
            dn = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
            assert re.search(r"\bT x264gpu_mbtree_pack\b", dn) and re.search(r"\bT x264gpu_mbtree_unpack\b", dn)

"""Batch groups that carry their members' side inputs, without a GPU: the gather entry is declared, bound, exported and resolved weakly by the host library; over
the CPU stand-in (which has no gather entry: the group copies row by row) sessions with --aq-mode 2 / 3 and --direct temporal write in a group what they write
alone.  The stand-in's x264gpu_encoder_set_lowres_mvs takes vectors for one stream only, so a group with macroblock-tree is covered on the device
(tests/test_gpu_batch_side_inputs.py), not here."""
import json
import os
import re
import subprocess
import sys

import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)


def test_gather_entry_is_declared_bound_and_exported():
    dev_h = open(os.path.join(ROOT, "include", "x264gpu.h")).read()
    assert re.search(r"int\s+x264gpu_gather_rows\s*\(const void \*const \*d_rows, size_t row_bytes, void \*d_dst, int rows, void \*stream\);", dev_h)
    assert "#define X264GPU_ABI_VERSION 2" in dev_h
    lib_py = open(os.path.join(ROOT, "x264vfw_amd", "lib.py")).read()
    assert re.search(r'"x264gpu_gather_rows": \(_i, \[_vp, _sz, _vp, _i, _vp\]\)', lib_py)
    unit = open(os.path.join(ROOT, "x264vfw_amd", "csrc", "gather.hip")).read()
    assert "int x264gpu_gather_rows(" in unit and "__shared__" not in unit and not re.search(r"atomic\w*\s*\(", unit)
    so = os.path.join(ROOT, "x264vfw_amd", "libx264gpu.so")
    assert os.path.exists(so), "the device library is built by build()"
    dn = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
    assert re.search(r"\bT x264gpu_gather_rows\b", dn)


def test_host_library_resolves_the_gather_entry_weakly():
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    libs = [os.path.join(HERE, "stub", "_build", "libx264gpu_host.so")]
    if os.path.exists(os.path.join(ROOT, "x264vfw_amd", "libx264gpu_host.so")):
        libs.append(os.path.join(ROOT, "x264vfw_amd", "libx264gpu_host.so"))
    for so in libs:
        nm = subprocess.run(["nm", "-D", so], capture_output=True, text=True, check=True).stdout
        assert re.search(r"^\s+w x264gpu_gather_rows$", nm, re.M), so
    stub = subprocess.run(["nm", "-D", os.path.join(HERE, "stub", "_build", "libx264gpu.so")], capture_output=True, text=True, check=True).stdout
    assert "x264gpu_gather_rows" not in stub, "the stand-in has no gather entry: the sessions below take the row-by-row path"


def _run(n, opts):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    r = subprocess.run([sys.executable, os.path.join(HERE, "stub", "run_host_batch_side.py"), str(n), "64", "48", "10"] + opts, capture_output=True, text=True, timeout=600)
    assert r.returncode == 0, r.stderr[-2000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


BASE = ["crf=24", "keyint=8", "min-keyint=8", "scenecut=0", "b-adapt=0", "bframes=2", "rc-lookahead=4", "no-mbtree"]


@pytest.mark.parametrize("mode", [2, 3])
def test_aq_modes_in_a_group_over_the_row_by_row_path(mode):
    """four sessions with --aq-mode 2 / 3 on different content in one group: the mode is kept, the group carries their offsets, the bytes are the solo sessions'"""
    info = _run(4, BASE + [f"aq-mode={mode}"])
    assert info["equal"] == [True] * 4 and all(info["sizes"]) and info["distinct"] == 4
    assert "B" in info["types"] or "R" in info["types"]
    for s in range(4):
        assert info["eff"][s]["aq_mode"] == mode == info["solo_eff"][s]["aq_mode"]
        assert any("X264GPU_BATCH: stream" in t and "the group carries each member's quantiser offsets" in t for t in info["log"][s]), info["log"][s]
        assert not any("runs on its own" in t or "aq-mode 1" in t for t in info["log"][s])


def test_temporal_direct_in_a_group():
    info = _run(2, BASE + ["direct=temporal"])
    spatial = _run(2, BASE + ["direct=spatial"])
    assert info["equal"] == [True, True] and all(e["direct"] == 2 for e in info["eff"])
    assert info["sizes"] != spatial["sizes"], "temporal direct prediction changed nothing"
    auto = _run(2, BASE + ["direct=auto"])
    assert all(e["direct"] == 1 for e in auto["eff"]) and auto["sizes"] == spatial["sizes"]


def test_a_tree_session_is_admitted_to_a_group():
    """the rule, without pictures: a session with macroblock-tree joins a group (the parent told it to run on its own) and reports the tree"""
    code = ("import os, sys, ctypes as C\n"
            "os.environ['X264_HOST_STUB'] = '1'; os.environ['X264GPU_BATCH'] = '2'\n"
            f"sys.path.insert(0, {HERE!r}); sys.path.insert(0, {ROOT!r})\n"
            "import host_lib as HL\n"
            "from quality_sessions import make_logger\n"
            "H = HL.H; p = HL.Param(); H.x264_param_default_preset(C.byref(p), b'medium', None)\n"
            "p.i_width, p.i_height, p.i_csp, p.i_fps_num, p.i_fps_den = 64, 48, HL.X264_CSP_I420, 25, 1\n"
            "for k, v in (('crf', '24'), ('keyint', '8'), ('scenecut', '0'), ('b-adapt', '0'), ('bframes', '2'), ('rc-lookahead', '4')):\n"
            "    assert H.x264_param_parse(C.byref(p), k.encode(), v.encode()) == 0\n"
            "log = []; cb = make_logger(log); p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2\n"
            "h = H.x264_encoder_open_157(C.byref(p)); assert h\n"
            "e = HL.Param(); H.x264_encoder_parameters(h, C.byref(e)); H.x264_encoder_close(h)\n"
            "import json; print(json.dumps({'mbtree': e.rc.b_mb_tree, 'log': [t for _, t in log]}))\n")
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    r = subprocess.run([sys.executable, "-c", code], capture_output=True, text=True, timeout=120)
    assert r.returncode == 0, r.stderr[-2000:]
    info = json.loads(r.stdout.strip().splitlines()[-1])
    assert info["mbtree"] == 1
    assert any("X264GPU_BATCH: stream 0 of a batch of 2" in t and "quantiser offsets and lookahead vectors" in t for t in info["log"]), info["log"]
    assert not any("runs on its own" in t for t in info["log"])

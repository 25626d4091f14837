"""CPU: noise reduction in every inter toolset (x264gpu_encoder_set_nr_any, X264GPU_NR_ANY=1) — the entry is declared, bound and exported; the host over a
device library without it (the tests' stand-in) falls back to the rules and messages it has without the variable; the new kernels' launch sites stay out of the
table of tests/mb_instantiations.py (nr_any_slice_*.hip / mb_launch_nr_any) and are the siblings the table lacks.  The device side: tests/test_gpu_nr_any.py."""
import ctypes as C
import glob
import json
import os
import re
import subprocess
import sys

import mb_instantiations as T
import test_mb_instantiations_cpu as TI

HERE = os.path.dirname(os.path.abspath(__file__))
ROOT = os.path.dirname(HERE)
NAME = "x264gpu_encoder_set_nr_any"


def test_header_declares_binding_exports_and_library_holds_the_entry():
    hdr = open(os.path.join(ROOT, "include", "x264gpu.h")).read()
    assert re.search(r"\bint\s+" + NAME + r"\s*\(", hdr), f"{NAME} is not declared in include/x264gpu.h"
    from x264vfw_amd import lib
    assert NAME in lib.EXPORTS and lib.x264gpu_encoder_set_nr_any.argtypes == lib.x264gpu_encoder_set_nr.argtypes
    so = C.CDLL(os.path.join(ROOT, "x264vfw_amd", "libx264gpu.so"))
    assert hasattr(so, NAME), f"libx264gpu.so lacks {NAME}"


def test_the_table_is_still_the_mb_slice_sites():
    """the existing completeness test, unedited: the new units are not mb_slice_*.hip and do not launch through mb_launch<"""
    TI.test_the_table_names_every_instantiation_and_no_other()


def test_the_new_launch_sites_are_the_siblings_the_table_lacks():
    site = re.compile(r"mb_launch_nr_any<([^>]*)>\s*\(")
    val = {"true": True, "false": False}
    found = []
    units = glob.glob(os.path.join(TI.CSRC, "nr_any_slice_*.hip"))
    for p in units:
        for args in site.findall(open(p).read()):
            a = [val[x] if x in val else int(x) for x in (s.strip() for s in args.split(","))]
            a += [0, False][len(a) - 2:]          # <M, ME, RD = 0, BS = false>
            found.append(T.mb_id(a[0], a[1], True, a[2], bool(a[3])))
    assert len(units) == 10 and len(found) == len(set(found)) == 38, (len(units), len(found))
    # every plain inter instantiation of the table (no psy-trellis) either has an NR sibling in the table or one here, never both
    plain_inter = {i for i in T.ALL_IDS if T.id_tuple(i)[2] and not T.id_tuple(i)[5] and not T.id_tuple(i)[6]}
    in_table = {i for i in plain_inter if (i | 1) in T.ALL_IDS}
    assert set(found) == plain_inter - in_table and len(in_table) == 18, (sorted(map(T.id_name, set(found) ^ (plain_inter - in_table))), len(in_table))


_CHILD = r"""
import ctypes as C, json, os, sys
os.environ["X264_HOST_STUB"] = "1"
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import host_lib as HL
import quality_sessions as S
H = HL.H
def eff_nr(preset, opts):
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), preset, None) == 0
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
    H.x264_encoder_close(h)
    return {"nr": eff.analyse.i_noise_reduction, "log": log}
base = {"qp": 26, "keyint": 30, "bframes": 2, "b-adapt": 0, "me": "hex", "subme": 7, "trellis": 1, "nr": 200}
print(json.dumps({"medium": eff_nr(b"medium", base), "ultrafast": eff_nr(b"ultrafast", {"nr": 200}), "dia": eff_nr(b"medium", dict(base, me="dia"))}))
"""


def _sessions(env):
    subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])
    e = dict(os.environ)
    e.pop("X264GPU_NR_ANY", None)
    e.update(env)
    r = subprocess.run([sys.executable, "-c", _CHILD, HERE], capture_output=True, text=True, timeout=600, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _nr_lines(log):
    return [t for lvl, t in log if "nr (noise reduction)" in t or "extended toolset" in t]


def test_host_over_the_stand_in_falls_back_with_the_variable_set():
    """the stand-in lacks every nr entry: with X264GPU_NR_ANY=1 each session reports nr 0 with the "device library" line, and nothing speaks of the extended toolset"""
    with_var, without = _sessions({"X264GPU_NR_ANY": "1"}), _sessions({})
    for name in ("medium", "ultrafast", "dia"):
        a = with_var[name]
        lines = _nr_lines(a["log"])
        assert a["nr"] == 0 and len(lines) == 1 and "a device library with the nr entries" in lines[0] and lines[0].rstrip().endswith("nr 0"), (name, a["log"])
        assert a == without[name], f"{name}: over a device library without the entry the variable changes nothing"

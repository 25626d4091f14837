"""CPU tests of GOP slots with quantisers planned ahead (X264GPU_GOP_SLOTS_RC=1: a CRF session with B pictures under --threads G keeps its B pictures, AQ mode,
macroblock-tree and rc-lookahead; host/gopslots.hpp put_planned), on the stand-in device library of tests/stub/ at 96x80: with the variable set the stream, the
picture types, pts / dts and nal_ref_idc equal the --threads 1 session of the same options, and x264host_gop_slots_planned says the path ran.

The stand-in takes the lookahead's vectors for encoders of ONE stream only (tests/stub/x264gpu_stub.c x264gpu_encoder_set_lowres_mvs: "lowres vectors: one stream
in the stub").  GopSlots::open asks the device library and, where it refuses, gives such a device's slots an encoder each (one INFO line): a macroblock-tree
session with several slots a device runs that way here (case 2) and in lock-step on one encoder, through the gather, on the device (tests/test_gpu_gop_slots_rc.py)."""
import functools
import json
import os
import subprocess
import sys

import numpy as np
import pytest

HERE = os.path.dirname(os.path.abspath(__file__))
RUN = os.path.join(HERE, "stub", "run_host_slots_rc.py")
subprocess.check_call(["make", "-s", "-C", os.path.join(HERE, "stub")])    # once, here: the child processes only load what it built
W, H_ = 96, 80

_C1 = {"crf": 24, "keyint": 8, "min-keyint": 8, "scenecut": 0, "bframes": 3, "b-adapt": 0, "weightp": 0, "ref": 2, "aq-mode": 1, "no-mbtree": None}
# number -> (options, pictures, seed, threads, stand-in devices); the options of 3 .. 6 are case 1's with what the case names changed
CASES = {
    1: (_C1, 23, 11, 3, 2),                                                                                    # two full GOPs and a shorter one
    2: (dict(_C1, crf=23, mbtree=None, **{"rc-lookahead": 6, "keyint": 9, "min-keyint": 9}, weightp=2, ref=3), 27, 11, 4, 3),
    3: (dict(_C1, **{"aq-mode": 3, "b-pyramid": "none"}, bframes=2), 21, 11, 2, 2),                            # the shorter GOP sits in the batch's last slot
    4: (dict(_C1, direct="temporal", mbtree=None, keyint=6, **{"min-keyint": 6}), 14, 11, 4, 4),               # one partly gathered batch; a slot a device
    5: (dict(_C1, keyint=12, **{"min-keyint": 12}), 5, 11, 2, 1),                                              # fewer pictures than one GOP
    6: (dict(_C1, bframes=1, slices=2, keyint=7, **{"min-keyint": 7}), 41, 11, 3, 2),                          # several batches
}
for _o in (CASES[2][0], CASES[4][0]):
    _o.pop("no-mbtree")


@functools.lru_cache(maxsize=None)
def _run(key, tmp, n, seed, devices, rc, fade=0):
    opts = dict(json.loads(key))
    env = dict(os.environ, X264GPU_STUB_DEVICES=str(devices))
    for k in ("X264GPU_DEVICES", "X264GPU_INFLIGHT", "X264GPU_BATCH", "X264GPU_GOP_SLOTS_RC"):
        env.pop(k, None)
    if rc:
        env["X264GPU_GOP_SLOTS_RC"] = "1"
    out_path = os.path.join(tmp, "s%08x.h264" % (hash((key, n, seed, devices, rc, fade)) & 0xffffffff))
    args = [sys.executable, RUN, out_path, str(W), str(H_), str(n), str(seed)] + [k if v is None else f"{k}={v}" for k, v in opts.items()] + ([f"fade={fade}"] if fade else [])
    out = subprocess.run(args, env=env, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    res = json.loads(out.stdout.decode().strip().splitlines()[-1])
    res["path"] = out_path
    return res


def run(tmp, opts, n, seed, devices, rc, fade=0):
    return _run(json.dumps(sorted(opts.items(), key=lambda kv: kv[0])), str(tmp), n, seed, devices, rc, fade)


@pytest.fixture(scope="module")
def tmp(tmp_path_factory):
    return tmp_path_factory.mktemp("slots_rc")


@pytest.mark.parametrize("case", sorted(CASES))
def test_planned_gop_slots_equal_the_serial_session(tmp, case):
    """bytes, picture types, pts / dts and nal_ref_idc of the --threads G session with the variable set are the --threads 1 session's; every picture was planned ahead.
    Case 2 (four slots on three devices with macroblock-tree): device 0 owns two slots, which the stand-in makes an encoder each (the module's docstring)."""
    opts, n, seed, threads, devices = CASES[case]
    serial = run(tmp, dict(opts, threads=1), n, seed, 1, False)
    par = run(tmp, dict(opts, threads=threads), n, seed, devices, True)
    assert par["frames"] == serial["frames"] == n
    assert sorted(serial["pts"]) == list(range(n)) and serial["pts"] != sorted(serial["pts"]), "the serial session codes B pictures"
    assert par["threads"] == threads and par["bframes"] == serial["bframes"] == opts["bframes"] and par["rc_method"] == serial["rc_method"]
    assert (par["mbtree"], par["lookahead"], par["aq_mode"], par["direct"]) == (serial["mbtree"], serial["lookahead"], serial["aq_mode"], serial["direct"])
    assert par["planned"] == n and serial["planned"] == 0
    assert any("quantisers planned ahead" in text for lvl, text in par["log"] if lvl == 2)
    assert par["sha"] == serial["sha"], "GOP slots with quantisers planned ahead: the stream differs from the serial one"
    assert (par["types"], par["pts"], par["dts"], par["ref_idc"]) == (serial["types"], serial["pts"], serial["dts"], serial["ref_idc"])
    assert par["meta"] == serial["meta"]
    assert sum(1 for c in par["calls"] if c > 0) == min(devices, threads, -(-n // opts["keyint"]))
    assert any("GOP slots run on an encoder each" in text for lvl, text in par["log"]) == (case == 2)


def test_case_2_with_a_slot_a_device(tmp):
    """case 2's session (macroblock-tree, rc-lookahead 6, --weightp 2's duplicates) on four stand-in devices: a slot a device, no device falls back to an encoder a slot"""
    opts, n, seed, threads, _ = CASES[2]
    serial = run(tmp, dict(opts, threads=1), n, seed, 1, False)
    par = run(tmp, dict(opts, threads=threads), n, seed, 4, True)
    assert par["planned"] == n and par["mbtree"] == serial["mbtree"] == 1 and par["lookahead"] == serial["lookahead"] == 6
    assert par["sha"] == serial["sha"] and par["meta"] == serial["meta"]
    assert not any("GOP slots run on an encoder each" in text for lvl, text in par["log"])


@pytest.mark.parametrize("case", [1, 2])
def test_the_serial_sessions_quantisers_vary(tmp, case):
    """not vacuous: the serial session's per-picture quantisers take at least three values (a slot that coded at its picture type's constant would show)"""
    opts, n, seed, _, _ = CASES[case]
    serial = run(tmp, dict(opts, threads=1), n, seed, 1, False)
    assert len(serial["qps"]) == n and len(set(serial["qps"])) >= 3, serial["qps"]


@pytest.mark.parametrize("case", [2, 3])
def test_the_serial_sessions_offset_rows_differ(tmp, case):
    """not vacuous: under macroblock-tree (case 2) and --aq-mode 3 (case 3) every picture comes with a quantiser-offset row, and the rows of two pictures differ"""
    opts, n, seed, _, _ = CASES[case]
    serial = run(tmp, dict(opts, threads=1), n, seed, 1, False)
    assert None not in serial["offsets"] and len(set(serial["offsets"])) >= 2, serial["offsets"]


def test_without_the_variable_the_session_is_downgraded_as_before(tmp):
    """case 1's options without X264GPU_GOP_SLOTS_RC: the warning, bframes 0, nothing planned ahead — and a stream that is not the serial session's"""
    opts, n, seed, threads, devices = CASES[1]
    serial = run(tmp, dict(opts, threads=1), n, seed, 1, False)
    off = run(tmp, dict(opts, threads=threads), n, seed, devices, False)
    assert any(lvl == 1 and text == "B-frames need %s in the MI355X path: bframes 0" for lvl, text in off["log"])
    assert off["bframes"] == 0 and off["planned"] == 0 and off["frames"] == n
    assert off["sha"] != serial["sha"]
    assert not any("planned ahead" in text for lvl, text in off["log"])


def test_a_fade_is_coded_unweighted_and_decodes_to_the_slots_reconstruction(tmp):
    """--weightp 2 on a clip that fades by 4 % a picture, macroblock-tree on: the lookahead weighs the fade for its costs, the slots code it without explicit weights
    (one INFO line says so), so the stream is not the serial session's — which codes weights — and the checker's decoder rebuilds what the slots reconstructed:
    the picture every slot coded last, at the end of its GOP's chain of references"""
    import oracle_lib as O
    opts = {"crf": 23, "keyint": 6, "min-keyint": 6, "scenecut": 0, "bframes": 3, "b-adapt": 0, "weightp": 2}
    n, G = 18, 3                                                      # one batch: slot s coded GOP s, its last picture in coding order is output picture 6 s + 5
    serial = run(tmp, dict(opts, threads=1), n, 11, 1, False, fade=4)
    par = run(tmp, dict(opts, threads=G), n, 11, G, True, fade=4)
    assert any(lvl == 2 and "in GOP slots: a fade's explicit weights are not coded" in text for lvl, text in par["log"])
    assert par["planned"] == n and par["frames"] == n and par["mbtree"] == 1 and par["weightp"] == 2
    assert (par["types"], par["pts"], par["dts"]) == (serial["types"], serial["pts"], serial["dts"])
    dec = O.h264_decode(open(par["path"], "rb").read(), n, W, H_)
    assert len(dec) == n
    assert par["sha"] != serial["sha"]
    recon = np.fromfile(par["path"] + ".recon", np.uint8).reshape(G, -1)
    for s in range(G):
        np.testing.assert_array_equal(dec[6 * s + 5], recon[s], err_msg=f"slot {s}: the decoder's picture {6 * s + 5} is not the slot's reconstruction")

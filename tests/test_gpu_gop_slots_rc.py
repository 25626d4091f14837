"""-m gpu: GOP slots with quantisers planned ahead (X264GPU_GOP_SLOTS_RC=1, host/gopslots.hpp put_planned) on the device, 96x80.  The sessions are those of
tests/test_gop_slots_rc_cpu.py: cases 2 (macroblock-tree, rc-lookahead 6, --weightp 2: offsets and lookahead vectors gathered for several slots of ONE device
encoder) and 3 (--aq-mode 3) equal the checker session — the stand-in build over the oracle at --threads 1 — byte for byte, as
test_gpu_host.py::test_gop_slots_with_b_pictures_equal_serial compares; case 1 on the device with --threads 3 equals the device's --threads 1 session."""
import functools
import hashlib
import json
import os
import subprocess
import sys

import pytest

import host_lib as HL

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(HERE, "stub"))
import run_host_slots_rc as R  # noqa: E402
from test_gop_slots_rc_cpu import CASES, W, H_  # noqa: E402  (also builds the stand-in)

pytestmark = pytest.mark.gpu


def device_session(monkeypatch, opts, n, seed, rc):
    for k in ("X264GPU_DEVICES", "X264GPU_INFLIGHT", "X264GPU_BATCH", "X264GPU_GOP_SLOTS_RC"):
        monkeypatch.delenv(k, raising=False)
    if rc:
        monkeypatch.setenv("X264GPU_GOP_SLOTS_RC", "1")
    return R.session(HL, None, W, H_, n, seed, opts, stub=False)


@functools.lru_cache(maxsize=None)
def checker_session(case):
    opts, n, seed, _, _ = CASES[case]
    env = dict(os.environ, X264GPU_STUB_DEVICES="1")
    for k in ("X264GPU_DEVICES", "X264GPU_INFLIGHT", "X264GPU_BATCH", "X264GPU_GOP_SLOTS_RC", "X264GPU_HOST_LIB"):
        env.pop(k, None)
    args = [sys.executable, os.path.join(HERE, "stub", "run_host_slots_rc.py"), "", str(W), str(H_), str(n), str(seed)] + [k if v is None else f"{k}={v}" for k, v in dict(opts, threads=1).items()]
    out = subprocess.run(args, env=env, capture_output=True, timeout=600)
    assert out.returncode == 0, out.stderr.decode()[-2000:]
    return json.loads(out.stdout.decode().strip().splitlines()[-1])


@pytest.mark.parametrize("case", [2, 3])
def test_planned_gop_slots_on_the_device_equal_the_checker_session(gpu, monkeypatch, case):
    opts, n, seed, threads, _ = CASES[case]
    ref = checker_session(case)
    par = device_session(monkeypatch, dict(opts, threads=threads), n, seed, True)
    assert par["planned"] == n and par["frames"] == ref["frames"] == n and par["threads"] == threads
    assert not any("GOP slots run on an encoder each" in text for lvl, text in par["log"]), "the device library takes per-stream vectors: the slots run in lock-step"
    assert (par["bframes"], par["mbtree"], par["lookahead"], par["aq_mode"]) == (ref["bframes"], ref["mbtree"], ref["lookahead"], ref["aq_mode"])
    assert len(set(ref["qps"])) >= 3 and None not in ref["offsets"] and len(set(ref["offsets"])) >= 2
    assert hashlib.sha256(par["stream"]).hexdigest() == ref["sha"], "GOP slots with quantisers planned ahead on the device: the stream differs from the checker session's"
    assert (par["types"], par["pts"], par["dts"], par["ref_idc"]) == (ref["types"], ref["pts"], ref["dts"], ref["ref_idc"])


def test_case_1_on_the_device_equals_the_devices_serial_session(gpu, monkeypatch):
    opts, n, seed, threads, _ = CASES[1]
    serial = device_session(monkeypatch, dict(opts, threads=1), n, seed, False)
    par = device_session(monkeypatch, dict(opts, threads=threads), n, seed, True)
    assert serial["planned"] == 0 and par["planned"] == n and par["bframes"] == serial["bframes"] == 3 and par["threads"] == threads
    assert len(set(serial["qps"])) >= 3
    assert par["stream"] == serial["stream"]
    assert par["meta"] == serial["meta"] and par["pts"] != sorted(par["pts"])

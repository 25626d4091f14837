"""-m gpu: the macroblock-tree statistics file on the device — the two entries of csrc/mbtree_stats.hip against the twin (tests/mbtree_stats_ref.py), a first and
a second pass of the host library over the device against the same sessions over the CPU stand-in, and the driver's multipass encode with the file switched on.

Rate accuracy of the driver's second pass (120 pictures 176x144, 300 kbit/s; profiles/mbtree_2pass.md has the measured figures): the tree pass' deviation from the
requested rate must be at most the larger of 0.05 and twice the deviation of the tree-less second pass of the same clip."""
import json
import os
import subprocess
import sys

import numpy as np
import pytest

import mbtree_sessions as S
import mbtree_stats_ref as R

pytestmark = pytest.mark.gpu
HERE = os.path.dirname(os.path.abspath(__file__))
W, H, KBPS = 176, 144, 200
KNOWN = [0.0, -0.0, 1 / 256, -1 / 256, 0.999 / 256, -0.999 / 256, 1.5, -1.5, 127.99609375, 200.0, -200.0, float("nan")]


def _pool():
    rng = np.random.default_rng(21)
    return np.concatenate([np.array(KNOWN, np.float32), rng.uniform(-300, 300, 64).astype(np.float32), rng.uniform(-40, 40, 4096).astype(np.float32)])


def _dev_pack(gpu, x):
    import torch
    d_x = torch.from_numpy(np.ascontiguousarray(x, np.float32)).cuda()
    d_w = torch.zeros(x.size, dtype=torch.int16, device="cuda")
    gpu.check(gpu.x264gpu_mbtree_pack(d_x.data_ptr(), x.size, d_w.data_ptr(), None), "mbtree_pack")
    torch.cuda.synchronize()
    return d_w.cpu().numpy().view(np.uint16).view(">i2")          # the bytes as they lie in memory = on the wire


def _dev_unpack(gpu, words):
    import torch
    raw = np.frombuffer(np.asarray(words, ">i2").tobytes(), np.int16)
    d_w = torch.from_numpy(raw.copy()).cuda()
    d_x = torch.zeros(raw.size, dtype=torch.float32, device="cuda")
    gpu.check(gpu.x264gpu_mbtree_unpack(d_w.data_ptr(), raw.size, d_x.data_ptr(), None), "mbtree_unpack")
    torch.cuda.synchronize()
    return d_x.cpu().numpy()


# ---- 1: the primitives ----
@pytest.mark.parametrize("n", [1, 63, 64, 65, 99, 257, 8160])
def test_pack_unpack_equal_the_twin(gpu, n):
    x = np.resize(_pool(), n)
    want = R.pack(x)
    got = _dev_pack(gpu, x)
    assert got.tobytes() == want.tobytes()
    back = _dev_unpack(gpu, got)
    assert back.tobytes() == R.unpack(want).tobytes()


def test_whole_pool_and_every_word(gpu):
    x = _pool()
    assert _dev_pack(gpu, x).tobytes() == R.pack(x).tobytes()          # the known answers, +-300 (saturation), +-40
    assert _dev_pack(gpu, np.array(KNOWN, np.float32)).astype(np.int32).tolist() == [0, 0, 1, -1, 0, 0, 384, -384, 32767, 32767, -32768, 0]
    w = np.arange(-32768, 32768).astype(">i2")                          # every representable value once, one launch
    f = _dev_unpack(gpu, w)
    assert f.tobytes() == R.unpack(w).tobytes()
    assert _dev_pack(gpu, f).tobytes() == w.tobytes()                   # pack(unpack(w)) == w for all words


def test_refusals_launch_nothing(gpu):
    import torch
    d_x = torch.full((64,), 3.0, dtype=torch.float32, device="cuda")
    d_w = torch.full((64,), 0x1234, dtype=torch.int16, device="cuda")
    E = -1          # X264GPU_EINVAL
    assert gpu.x264gpu_mbtree_pack(None, 64, d_w.data_ptr(), None) == E
    assert gpu.x264gpu_mbtree_pack(d_x.data_ptr(), 64, None, None) == E
    assert gpu.x264gpu_mbtree_pack(d_x.data_ptr(), 0, d_w.data_ptr(), None) == E
    assert gpu.x264gpu_mbtree_unpack(None, 64, d_x.data_ptr(), None) == E
    assert gpu.x264gpu_mbtree_unpack(d_w.data_ptr(), 64, None, None) == E
    assert gpu.x264gpu_mbtree_unpack(d_w.data_ptr(), 0, d_x.data_ptr(), None) == E
    assert gpu.x264gpu_mbtree_unpack(d_w.data_ptr(), -5, d_x.data_ptr(), None) == E
    torch.cuda.synchronize()
    assert bool((d_x == 3.0).all()) and bool((d_w == 0x1234).all())          # nothing was written


# ---- 2 and 3: the sessions, on the device and over the CPU stand-in ----
class World:
    pass


@pytest.fixture(scope="module")
def world(gpu, tmp_path_factory):
    wd = World()
    wd.dev, wd.cpu = tmp_path_factory.mktemp("mbtree_dev"), tmp_path_factory.mktemp("mbtree_cpu")
    # one child process over the device, one over the CPU stand-in: the first pass in a directory of its own, then the second pass over the DEVICE's two files
    # (the device child also runs the first pass' session without pass=1)
    st = wd.dev / "x264.stats"
    p2 = [f"stats={st}", f"bitrate={KBPS}", "pass=2", "plan=1"]
    wd.p1, wd.plain, wd.p2 = S.run_many([(wd.dev / "p1.h264", W, H, [f"stats={st}", "crf=24", "pass=1"], True), (wd.dev / "plain.h264", W, H, ["crf=24"], False),
                                         (wd.dev / "p2.h264", W, H, p2, True)], True, device=True)
    wd.p1_cpu, wd.p2_cpu = S.run_many([(wd.cpu / "p1.h264", W, H, [f"stats={wd.cpu / 'x264.stats'}", "crf=24", "pass=1"], True), (wd.cpu / "p2.h264", W, H, p2, True)], True, device=False)
    return wd


def test_first_pass_on_the_device(world):
    info, stream, offs = world.p1
    S.check_first_pass(W, H, world.dev / "x264.stats", info, stream, offs, world.plain[1], "device")
    assert any("packed on the host" in t for t in S.texts(world.p1_cpu[0]))
    # the stand-in's session wrote the same file for the same clip (the device's lookahead is bit-exact against the oracle's), and the same statistics
    assert (world.dev / "x264.stats.mbtree").read_bytes() == (world.cpu / "x264.stats.mbtree").read_bytes()
    assert (world.dev / "x264.stats").read_bytes() == (world.cpu / "x264.stats").read_bytes()
    assert stream == world.p1_cpu[1]


def test_second_pass_on_the_device(world):
    info, stream, offs = world.p2
    S.check_second_pass(W, H, world.dev / "x264.stats", KBPS, info, stream, offs, world.p1[0], world.p1[2], "device")
    # the stand-in's second pass over the same two files
    _i, cpu_stream, cpu_offs = world.p2_cpu
    assert any("unpacked on the host" in t for t in S.texts(_i))
    assert all((a is None and b is None) or np.array_equal(a, b) for a, b in zip(offs, cpu_offs))
    assert stream == cpu_stream


# ---- 4: the driver ----
def test_multipass_through_the_driver_with_the_tree_file(gpu, tmp_path):
    """the existing driver test's clip and options (tests/test_gpu_vfw.py::test_two_pass_through_the_driver) at half its length — 120 pictures: three keyint-40 GOPs and
    nearly five times the 25 coded pictures after which the second pass' feedback starts (rate_estimate_qscale: h->i_frame >= fps) — in one child process that has the
    variable in its environment.  Four passes of 120 pictures through the driver: about 15 s, what this test is about (the existing driver test takes 27 s)"""
    w, h, nfr, kbps = 176, 144, 120, 300
    r = subprocess.run([sys.executable, os.path.join(HERE, "vfw_mbtree_child.py"), str(tmp_path), str(w), str(h), str(nfr), str(kbps)], capture_output=True, text=True, timeout=600,
                       env=dict(os.environ, X264GPU_MBTREE_STATS="1"))
    assert r.returncode == 0, r.stderr[-3000:]
    res = json.loads(r.stdout.strip().splitlines()[-1])
    tree, plain = res["tree"], res["plain"]
    assert tree["after_pass1"] == ["stats", "stats.mbtree"], tree["after_pass1"]          # pass 1: no stream (b_no_output), the two statistics files, no .temp
    assert "packed on the device" in tree["log1"], tree["log1"]
    assert os.path.getsize(tmp_path / "tree" / "stats.mbtree") == len(R.kept_lines(S.stat_lines(tmp_path / "tree" / "stats"))) * R.record_size(S.nmb_of(w, h))
    assert "planned from the first pass" in tree["log2"] and "from the macroblock-tree statistics file, unpacked on the device" in tree["log2"], tree["log2"]
    assert "mbtree 0" not in tree["log1"] + tree["log2"]
    assert plain["files"] == ["p2.h264", "stats"] and S.TODAY in plain["log1"] and S.TODAY in plain["log2"]
    dev_tree, dev_plain = abs(tree["rate"] / kbps - 1.0), abs(plain["rate"] / kbps - 1.0)
    print(f"second pass at {kbps} kbit/s: with the tree file {tree['rate']:.2f} kbit/s (deviation {dev_tree:.4f}), tree-less {plain['rate']:.2f} kbit/s (deviation {dev_plain:.4f})")
    assert dev_tree <= max(0.05, 2 * dev_plain), (tree["rate"], plain["rate"])
    import oracle_lib as O
    assert len(O.h264_decode((tmp_path / "tree" / "p2.h264").read_bytes(), nfr, w, h)) == nfr

"""-m gpu: batch groups whose members have lookaheads of their own — macroblock-tree, --aq-mode 2 / 3, --direct temporal.  The gather entry that builds a round's
[streams][mb_count] arrays against numpy; sessions under X264GPU_BATCH against the same sessions alone (bytes, log, reported parameters); that the side inputs
matter and that every stream receives its own; the round modes; groups that must not mix; the checker's decoder.
Pictures are 96x80 = 6x5 macroblocks: interior macroblocks have every neighbour, and a row of offsets is 120 bytes, no multiple of 16."""
import ctypes as C
import functools
import threading

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

W, H_, NMB, NF = 96, 80, 30, 10
TREE = {"crf": 24, "keyint": 8, "min-keyint": 8, "scenecut": 0, "b-adapt": 0, "bframes": 2, "rc-lookahead": 4}          # mbtree on: medium's default
CONFIGS = {
    "tree": TREE,
    "notree": dict(TREE, **{"no-mbtree": None}),
    "aq2": dict(TREE, **{"aq-mode": 2, "no-mbtree": None}),
    "aq3": dict(TREE, **{"aq-mode": 3, "no-mbtree": None}),
    "aq3tree": dict(TREE, **{"aq-mode": 3}),
    "temporal": dict(TREE, **{"direct": "temporal", "no-mbtree": None}),
    "spatial": dict(TREE, **{"direct": "spatial", "no-mbtree": None}),
    "auto": dict(TREE, **{"direct": "auto", "no-mbtree": None}),
}


# ---- (1) the gather entry ----
@pytest.mark.parametrize("rows", [1, 3, 67])
@pytest.mark.parametrize("row_bytes", [4, 120, 4096 + 12])
def test_gather_rows_against_numpy(gpu, rows, row_bytes):
    """sources carved out of one buffer at odd byte offsets (every alignment class against the destination rows: the same 16-byte phase, a multiple of four apart,
    anything), one of them null; the destination at an odd offset inside a guard pattern that must survive"""
    import torch
    rng = np.random.default_rng(rows * 10007 + row_bytes)
    pool = rng.integers(0, 256, rows * (row_bytes + 64) + 64, dtype=np.uint8)
    d_pool = torch.from_numpy(pool).cuda()
    guard, lead = 256, 3          # the destination starts 3 bytes past a 16-byte boundary: rows of 120 bytes then begin at every phase of 8 + 3
    d_dst = torch.full((guard + lead + rows * row_bytes + guard,), 0xA5, dtype=torch.uint8, device="cuda")
    base = d_dst.data_ptr() + guard + lead
    null_row = rows // 2
    offs, ptrs = [], []
    for r in range(rows):
        # row 0: the destination row's own phase (one vector load a piece); row 1: four bytes off (dwords); the others: any odd offset
        dphase = (base + r * row_bytes) % 16
        want = dphase if r % 3 == 0 else (dphase + 4) % 16 if r % 3 == 1 else int(rng.integers(0, 16)) | 1
        start = r * (row_bytes + 64) + 16
        start += (want - (d_pool.data_ptr() + start)) % 16
        offs.append(start)
        ptrs.append(0 if r == null_row and rows > 1 else d_pool.data_ptr() + start)
    d_tab = torch.from_numpy(np.array(ptrs, np.uint64).view(np.int64)).cuda()
    gpu.check(gpu.x264gpu_gather_rows(d_tab.data_ptr(), row_bytes, base, rows, None), "gather")
    torch.cuda.synchronize()
    got = d_dst.cpu().numpy()
    assert (got[:guard + lead] == 0xA5).all() and (got[guard + lead + rows * row_bytes:] == 0xA5).all(), "bytes outside the destination were written"
    body = got[guard + lead:guard + lead + rows * row_bytes].reshape(rows, row_bytes)
    for r in range(rows):
        want = np.zeros(row_bytes, np.uint8) if ptrs[r] == 0 else pool[offs[r]:offs[r] + row_bytes]
        assert np.array_equal(body[r], want), f"row {r} of {rows} x {row_bytes} bytes"


def test_gather_rows_refuses_bad_arguments(gpu):
    import torch
    d = torch.zeros(64, dtype=torch.uint8, device="cuda")
    t = torch.from_numpy(np.array([d.data_ptr()], np.uint64).view(np.int64)).cuda()
    EINVAL = -1
    assert gpu.x264gpu_gather_rows(None, 16, d.data_ptr() + 32, 1, None) == EINVAL
    assert gpu.x264gpu_gather_rows(t.data_ptr(), 16, None, 1, None) == EINVAL
    assert gpu.x264gpu_gather_rows(t.data_ptr(), 16, d.data_ptr() + 32, 0, None) == EINVAL
    assert gpu.x264gpu_gather_rows(t.data_ptr(), 0, d.data_ptr() + 32, 1, None) == EINVAL
    torch.cuda.synchronize()
    assert not d.cpu().numpy().any()


# ---- sessions ----
def _session(opts, frames, recon=False):
    """one session through x264_encoder_encode -> dict(stream, log, eff = what x264_encoder_parameters reports, offs = after every call the offsets the hook
    x264host_last_mb_qp_offsets hands back (None: none), recons)"""
    import host_lib as HL
    from quality_sessions import make_logger
    H = HL.H
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", None) == 0
    p.i_width, p.i_height, p.i_csp = W, H_, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 3
    p.b_vfr_input = 0
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_, "x264_encoder_open failed"
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, W, H_) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    res = dict(stream=b"", log=log, offs=[], recons=[], eff=dict(mbtree=eff.rc.b_mb_tree, aq_mode=eff.rc.i_aq_mode, direct=eff.analyse.i_direct_mv_pred))

    def take(size):
        assert size >= 0, log[-3:]
        o = np.zeros(NMB, np.float32)
        res["offs"].append(o if H.x264host_last_mb_qp_offsets(h_, o.ctypes.data, NMB) == NMB else None)
        if size:
            res["stream"] += C.string_at(nal[0].p_payload, size)
            if recon:
                rec = np.zeros(W * H_ * 3 // 2, np.uint8)
                assert H.x264host_get_recon(h_, rec.ctypes.data) == 0
                res["recons"].append(rec)
    for i, f in enumerate(frames):
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out)))
    while H.x264_encoder_delayed_frames(h_):
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out)))
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return res


def _frames(i):
    from test_gpu_b_pred_reuse import static_frames
    return static_frames(W, H_, NF, 60 + i, 4)


@functools.lru_cache(maxsize=None)
def _solo(name, i, recon=False):
    """session i (content i) of a configuration on its own: computed once, shared by the tests, never changed"""
    return _session(CONFIGS[name], _frames(i), recon=recon)


def _together(n, names, env=None):
    """one session per entry of `names` (session i codes content i) from as many threads under X264GPU_BATCH=n"""
    from test_gpu_quality import _with_env
    res, errs = [None] * len(names), []

    def one(i):
        try:
            res[i] = _session(CONFIGS[names[i]], _frames(i))
        except BaseException as e:  # noqa: BLE001
            errs.append(f"session {i}: {e!r}")
    ths = [threading.Thread(target=one, args=(i,)) for i in range(len(names))]
    _with_env(dict({"X264GPU_BATCH": str(n)}, **(env or {})), lambda: ([t.start() for t in ths], [t.join() for t in ths]))
    assert not errs, errs
    return res


@functools.lru_cache(maxsize=None)
def _six(name):
    """six sessions of one configuration under X264GPU_BATCH=3: two groups"""
    return _together(3, [name] * 6)


def _in_a_group(r):
    texts = [t for _, t in r["log"]]
    return any("X264GPU_BATCH: stream" in t for t in texts) and not any("runs on its own" in t for t in texts)


# ---- (2), (3), (4) batched equals alone ----
@pytest.mark.parametrize("name,mbtree,aq_mode", [("tree", 1, 1), ("aq2", 0, 2), ("aq3", 0, 3), ("aq3tree", 1, 3), ("temporal", 0, 1)])
def test_batched_sessions_code_what_they_code_alone(gpu, name, mbtree, aq_mode):
    """six sessions on different content in two groups of three: every session runs in a group, reports the tree / AQ mode / direct mode it asked for, and writes
    the bytes it writes alone"""
    together = _six(name)
    for i in range(6):
        a, b = together[i], _solo(name, i)
        assert _in_a_group(a), (i, a["log"])
        assert a["eff"]["mbtree"] == mbtree and a["eff"]["aq_mode"] == aq_mode and a["eff"] == b["eff"], (i, a["eff"], b["eff"])
        assert a["eff"]["direct"] == (2 if name == "temporal" else 1)
        assert not any("aq-mode 1" in t for _, t in a["log"]), a["log"]
        carries = any("the group carries each member's" in t for _, t in a["log"])
        assert carries == (name != "temporal"), a["log"]
        assert len(a["stream"]) > 0 and a["stream"] == b["stream"], f"session {i} ({name}) codes other bytes in its group than alone"
    assert len({r["stream"] for r in together}) == 6


def test_temporal_direct_is_used_and_auto_is_not(gpu):
    """the temporal sessions' streams differ from the same sessions with spatial direct prediction (so their B pictures were coded with the other mode);
    --direct auto in a batch runs spatial and says so"""
    temporal = _six("temporal")
    assert any(temporal[i]["stream"] != _solo("spatial", i)["stream"] for i in range(6)), "temporal direct prediction changed nothing"
    auto = _together(2, ["auto", "auto"])
    for i, r in enumerate(auto):
        assert _in_a_group(r) and r["eff"]["direct"] == 1, r["log"]
        assert any("direct auto: not in cross-session batches" in t for _, t in r["log"]) and not any("direct temporal" in t for _, t in r["log"]), r["log"]
        assert r["stream"] == _solo("spatial", i)["stream"]


# ---- (5) not vacuous ----
def test_side_inputs_matter_and_every_stream_has_its_own(gpu):
    tree = _six("tree")
    assert any(tree[i]["stream"] != _solo("notree", i)["stream"] for i in range(6)), "the tree changed no session's bytes"
    # the two members of one group, after the same call
    a, b = _together(2, ["tree", "tree"])
    assert _in_a_group(a) and _in_a_group(b) and a["stream"] == _solo("tree", 0)["stream"] and b["stream"] == _solo("tree", 1)["stream"]
    calls = [k for k in range(min(len(a["offs"]), len(b["offs"]))) if a["offs"][k] is not None and b["offs"][k] is not None]
    assert calls, "no call of the two sessions had offsets"
    assert any(a["offs"][k].any() and b["offs"][k].any() and not np.array_equal(a["offs"][k], b["offs"][k]) for k in calls)


# ---- (6) round modes ----
@pytest.mark.parametrize("env", [{"X264GPU_BATCH_ASYNC": "0"}, {"X264GPU_BATCH_OVERLAP": "0"}])
def test_round_modes(gpu, env):
    """rounds that are awaited instead of queued, and results downloaded in the call that submitted: the same bytes"""
    together = _together(3, ["tree"] * 3, env)
    for i in range(3):
        assert _in_a_group(together[i]), together[i]["log"]
        assert together[i]["stream"] == _solo("tree", i)["stream"], (env, i)


# ---- (7) groups do not mix ----
def test_tree_and_treeless_sessions_form_groups_of_their_own(gpu):
    names = ["tree", "notree", "tree", "notree"]
    together = _together(2, names)
    for i, r in enumerate(together):
        assert _in_a_group(r), r["log"]
        assert any("stream 0 of a batch of 2" in t or "stream 1 of a batch of 2" in t for _, t in r["log"])
        assert any("quantiser offsets and lookahead vectors" in t for _, t in r["log"]) == (names[i] == "tree"), r["log"]
        assert r["eff"]["mbtree"] == (names[i] == "tree")
        assert r["stream"] == _solo(names[i], i)["stream"], f"session {i} ({names[i]})"


# ---- (8) the checker decodes it ----
def test_checker_decodes_a_tree_session(gpu):
    """the solo session's reconstructions are what the checker's decoder makes of its stream — and the batched session writes the same stream"""
    s = _solo("tree", 0, True)
    assert len(s["recons"]) == NF
    dec = O.h264_decode(s["stream"], NF, W, H_)
    assert len(dec) == NF
    for k in range(NF):
        np.testing.assert_array_equal(dec[k], s["recons"][k], err_msg=f"decoded picture {k} != encoder reconstruction")
    assert _six("tree")[0]["stream"] == s["stream"]
    dec_b = O.h264_decode(_six("tree")[0]["stream"], NF, W, H_)
    assert len(dec_b) == NF

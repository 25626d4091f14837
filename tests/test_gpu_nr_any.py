"""-m gpu: noise reduction in every inter toolset (x264gpu_encoder_set_nr_any, X264GPU_NR_ANY=1): the NR siblings of the plain instantiations of the macroblock
loop — without RD, RD with CAVLC bit counts, RD with CABAC sizes under every search method, the trellis levels under me dia / esa — against the plain kernels
(zero offsets), the pure-Python twin (tests/nr_ref.py: statistics), offsets of 32767 (every final-encode site), the checker's decoder (device-ABI streams and
host sessions of the fast presets), and the batcher.  Helpers of tests/test_gpu_nr.py are reused by import."""
import json
import os
import subprocess
import sys
import threading

import numpy as np
import pytest

import bgop
import mb_instantiations as T
import nr_ref as N
import oracle_lib as O
import test_gpu_nr as G

pytestmark = pytest.mark.gpu

HERE = os.path.dirname(os.path.abspath(__file__))
W, H = 64, 48
ANY_BIT = 1 << 17          # x264gpu_mb_kernels_seen: an instantiation that only x264gpu_encoder_set_nr_any reaches
NORD = dict(rd=0, trellis=0, psy_rd_q8=0, subme=5)

# (name, what it changes in test_gpu_nr.MEDIUM, the search methods it is new under, M, RD of the P kernel, RD of the B kernel)
LEVELS = (("nord", NORD, (0, 1, 2, 3), 2, 0, 0),
          ("bigmargin", dict(NORD, subme=8), (0, 1, 2, 3), 5, 0, 0),          # --subme 8 without RD: the P kernel with the 5-sample margin (B slices: margin 2)
          ("cavlc", dict(cabac=0, trellis=0), (0, 1, 2, 3), 2, 1, 1),
          ("cabac", dict(trellis=0), (0, 1, 2, 3), 2, 2, 2),
          ("subme6", dict(subme=6), (0, 3), 2, 3, 7),
          ("trellis1", {}, (0, 3), 2, 3, 3),
          ("trellis2", dict(trellis=127), (0, 3), 2, 4, 4))
COMBOS = [(name, me) for name, _, mes, _, _, _ in LEVELS for me in mes]
BY_LEVEL = {l[0]: l for l in LEVELS}


def over_of(name, me):
    over = dict(BY_LEVEL[name][1], me_method=me)
    if me == 3:
        over["me_range"] = 8
    return over


def ids_of(name, me):
    """-> (the NR ids of the P and the B kernel with the set_nr_any bit, their plain siblings)"""
    _, _, _, M, rd_p, rd_b = BY_LEVEL[name]
    nr = {ANY_BIT | T.mb_id(M, me, True, rd_p, False, False, True), ANY_BIT | T.mb_id(2, me, True, rd_b, True, False, True)}
    return nr, {T.mb_id(M, me, True, rd_p), T.mb_id(2, me, True, rd_b, True)}


def test_the_new_instantiations_are_counted():
    """38 kernels: the 34 of the margin-2 table (RD 0 / 1 / 2 under four search methods, RD 3 / 4 / 7 under dia and esa) and the four P kernels with the 5-sample margin"""
    ids = set()
    for name, me in COMBOS:
        ids |= ids_of(name, me)[0]
    assert len(ids) == 38, sorted(hex(i) for i in ids)
    plain = {i & 0xffff & ~1 for i in ids}
    assert plain <= T.ALL_IDS and not {i | 1 for i in plain} & T.ALL_IDS, "every one is the sibling of a plain instantiation of the table that had none"


class AnySession(G.Session):
    """test_gpu_nr.Session through x264gpu_encoder_set_nr_any"""

    def __init__(self, lib, w, h, offsets=None, nr=True, **over):
        super().__init__(lib, w, h, offsets=offsets, nr=False, **over)
        self.nr = nr
        if nr:
            lib.check(lib.x264gpu_encoder_set_nr_any(self.gg.h, self.d_off.data_ptr(), self.d_pic.data_ptr()), "set_nr_any")


def seen(lib, reset=True):
    import ctypes as C
    buf = (C.c_uint32 * 256)()
    n = lib.x264gpu_mb_kernels_seen(buf, 256, 1 if reset else 0)
    return set(buf[:min(n, 256)])


# ---- (1) zero offsets are the plain kernels, on a P and on B pictures, and the NR kernels are the ones that ran ----
@pytest.mark.parametrize("name,me", COMBOS, ids=[f"{T.ME_NAMES[me]}-{name}" for name, me in COMBOS])
def test_zero_offsets_are_the_plain_kernels(gpu, name, me):
    frames = G.two_streams(W, H, 5, 31)
    over = over_of(name, me)
    nr_ids, plain_ids = ids_of(name, me)
    runs = []
    for nr in (False, True):
        seen(gpu)
        s = AnySession(gpu, W, H, nr=nr, **over)
        runs.append(s.code(frames, "IPBBP"))
        if nr:
            assert not s.offsets().any()
        s.close()
        ran = seen(gpu)
        if nr:
            assert nr_ids <= ran and not plain_ids & ran, f"kernels launched: {sorted(hex(i) for i in ran)}, wanted {sorted(hex(i) for i in nr_ids)}"
        else:
            assert plain_ids <= ran and not nr_ids & ran, f"the plain session launched {sorted(hex(i) for i in ran)}"
    G._same_pictures(runs[0], runs[1], f"{name} me {me}")
    assert any(p["sums"][s]["count"][c] for p in runs[1] for s in range(2) for c in range(3)), "the denoising kernels ran: some statistics"
    assert all(not any(p["sums"][s]["count"]) for p in runs[1] if p["pt"] <= 1 for s in range(2)), "an I picture has none"


def test_refinement_without_trellis_runs_the_first_nr_kernels(gpu):
    """--subme 9 --trellis 0 under me hex: a session x264gpu_encoder_set_nr refuses (no trellis) whose kernels — RD 5 — exist since that entry: set_nr_any admits it
    and launches them, with zero offsets byte for byte the plain session"""
    import torch
    frames = G.two_streams(W, H, 5, 31)
    over = dict(subme=9, rd=63, trellis=0, me_method=1)
    probe = AnySession(gpu, W, H, nr=False, **over)
    d_off, d_pic = torch.zeros((2, 192), dtype=torch.int16, device="cuda"), torch.zeros((2, 1552), dtype=torch.uint8, device="cuda")
    assert gpu.x264gpu_encoder_set_nr(probe.gg.h, d_off.data_ptr(), d_pic.data_ptr()) == -1
    probe.close()
    runs = []
    for nr in (False, True):
        seen(gpu)
        s = AnySession(gpu, W, H, nr=nr, **over)
        runs.append(s.code(frames, "IPBBP"))
        s.close()
        ran = seen(gpu)
    assert {T.mb_id(5, 1, True, 5, False, False, True), T.mb_id(5, 1, True, 5, True, False, True)} <= ran, sorted(hex(i) for i in ran)
    G._same_pictures(runs[0], runs[1], "refinement without trellis")


def test_a_session_of_the_first_toolset_keeps_its_kernels(gpu):
    """set_nr_any on a CABAC trellis session under me hex launches what set_nr launches there"""
    frames = G.two_streams(W, H, 5, 31)
    seen(gpu)
    s = AnySession(gpu, W, H, me_method=1)
    s.code(frames, "IPBBP")
    s.close()
    ran = seen(gpu)
    assert {T.mb_id(2, 1, True, 3, False, False, True), T.mb_id(2, 1, True, 3, True, False, True)} <= ran and not any(i & ANY_BIT for i in ran), sorted(hex(i) for i in ran)


# ---- (2) statistics equal the twin's ----
STAT_CASES = {"rd0-dia-cavlc": dict(NORD, cabac=0, me_method=0), "rd0-hex-cabac": dict(NORD, me_method=1), "rd1-hex": dict(cabac=0, trellis=0, me_method=1)}


@pytest.mark.parametrize("slices", [1, 3])
@pytest.mark.parametrize("case", sorted(STAT_CASES))
def test_statistics_equal_twin(gpu, case, slices):
    frames = G.two_streams(W, H, 3, 31)
    over = dict(STAT_CASES[case], refs=1)
    if slices > 1:
        over.update(slices=slices, slices_plain=1)
    s = AnySession(gpu, W, H, **over)
    pics = s.code(frames, "IPP", update=300)
    s.close()
    coded = 0
    for k in (1, 2):
        for st in range(2):
            mbs = pics[k]["mb"][st]
            coded += int(np.isin(mbs["type"], (O.MB_P_L0, O.MB_P_8x8)).sum())
            want = N.picture_sums(O, frames[st][pics[k]["disp"]], pics[k - 1]["recon"][st], mbs, W, H)
            got = pics[k]["sums"][st]
            assert got["count"] == want["count"], f"picture {k} stream {st}: counts {got['count']} twin {want['count']}"
            assert got["sum"] == want["sum"], f"picture {k} stream {st}: sums differ"
    assert coded >= 8, f"inter macroblocks that are no skips: {coded}"
    assert pics[2]["pic"] is not None and s.offsets().any(), "the second P picture was denoised with offsets that are not zero"


# ---- (3) every final-encode site denoises, per category, without RD and with CAVLC bit counts ----
SITE_CASES = {"rd0": dict(NORD, me_method=1), "rd1": dict(cabac=0, trellis=0, me_method=1)}


def _inter_levels_by_category(pics):
    """non-zero AC levels of the inter macroblocks of the P and B pictures per category (0 luma 4x4, 1 luma 8x8, 2 chroma), and the number of intra macroblocks"""
    n, intra = [0, 0, 0], 0
    for p in pics:
        if p["pt"] <= 1:
            continue
        for st in range(2):
            for m, lv in zip(p["mb"][st], p["lv"][st]):
                t = int(m["type"])
                if t in (O.MB_P_SKIP, O.MB_B_SKIP):
                    assert not lv.any()
                elif t >= O.MB_P_L0:
                    ac = lv[:256].reshape(16, 16).copy()
                    if m["transform8x8"]: ac[0::4, 0] = 0
                    else: ac[:, 0] = 0
                    n[1 if m["transform8x8"] else 0] += int(np.count_nonzero(ac))
                    n[2] += int(np.count_nonzero(lv[G.LV_CHROMA_AC:G.LV_CHROMA_AC + 128]))
                else:
                    intra += 1
    return n, intra


def _static_noisy(w, h, n, seed, luma, chroma):
    """test_gpu_b_pred_reuse.static_frames with noise on the chroma planes too: one picture of the synthetic content, fresh noise of +-luma / +-chroma on every frame —
    inter macroblocks with residual in all three categories"""
    from synth import synth_frames
    rng = np.random.default_rng(seed)
    base = synth_frames(w, h, 1, seed=seed)[0].astype(np.int32)
    amp = np.concatenate([np.full(w * h, luma), np.full(w * h // 2, chroma)])
    return [np.clip(base + rng.integers(-amp, amp + 1), 16, 235).astype(np.uint8) for _ in range(n)]


@pytest.fixture(scope="module")
def site_content():
    return [_static_noisy(96, 80, 5, 40 + s, 12, 8) for s in range(2)]


@pytest.fixture(scope="module")
def site_plain(gpu, site_content):
    """the plain runs: the content must leave inter levels in every category"""
    out = {}
    for case, over in SITE_CASES.items():
        s = AnySession(gpu, 96, 80, nr=False, **over)
        out[case] = _inter_levels_by_category(s.code(site_content, "IPBBP"))
        s.close()
    return out


@pytest.mark.parametrize("cats", [(0, 1, 2), (0,), (1,), (2,)])
@pytest.mark.parametrize("case", sorted(SITE_CASES))
def test_every_final_encode_site_denoises(gpu, site_content, site_plain, case, cats):
    plain, plain_intra = site_plain[case]
    print(f"{case}: the plain run's inter AC levels per category {plain}, intra macroblocks {plain_intra}")
    assert all(plain[c] > 0 for c in range(3)), f"the content leaves no inter level in some category without nr: {plain}"
    off = N.zero_offsets()
    for c in cats:
        off[c, 1:N.NCOEF[c]] = 32767
    s = AnySession(gpu, 96, 80, offsets=off, **SITE_CASES[case])
    pics = s.code(site_content, "IPBBP")
    s.close()
    ninter = 0
    for p in pics:
        if p["pt"] <= 1:
            continue
        for st in range(2):
            for m, lv in zip(p["mb"][st], p["lv"][st]):
                if int(m["type"]) >= O.MB_P_L0 and int(m["type"]) not in (O.MB_P_SKIP, O.MB_B_SKIP):
                    ok, _ = G._inter_ok(m, lv, cats)
                    assert ok, f"{case}: picture type {p['pt']} macroblock type {int(m['type'])}: AC levels survive offsets of 32767 in categories {cats}"
                    ninter += 1
    got, intra = _inter_levels_by_category(pics)
    print(f"{case} {cats}: inter AC levels per category {got} over {ninter} coded inter macroblocks, intra macroblocks {intra} (plain {plain_intra})")
    assert all(got[c] == 0 for c in cats)


# ---- (4) re-issue is exact without RD ----
def test_reissue_is_exact(gpu):
    frames = G.two_streams(W, H, 2, 31)
    off = G._offsets("random", np.random.default_rng(5))
    off[:] //= 30
    s = AnySession(gpu, W, H, offsets=off, **dict(NORD, me_method=0))
    s.code(frames, "I")
    order = bgop.schedule("IP", 1)
    pic, _ = s.dpb.plan(order[1][1], 1, ())
    got = []
    for qp in (23, 30, 23):
        pic.qp = qp
        mb, lv = s.gg.encode_pics([frames[0][1], frames[1][1]], [pic, pic])
        got.append((mb.tobytes(), lv.tobytes(), s.gg.recon(0).tobytes(), s.gg.recon(1).tobytes(), s.d_pic.cpu().numpy().tobytes()))
        np.testing.assert_array_equal(s.offsets(), np.broadcast_to(off, (2, 3, 64)))
    s.close()
    assert got[0] == got[2], "the same picture issued again gives other records, levels, reconstruction or statistics"
    assert got[0][:2] != got[1][:2], "another quantiser between: another picture"
    assert any(N.sums_from_bytes(got[0][4][:1552])["count"])


# ---- (5) the checker decodes device-ABI streams ----
ULTRAFAST = dict(cabac=0, me_method=0, subme=0, rd=0, trellis=0, psy_rd_q8=0, dct8x8=0, partitions=0, refs=1, mixed_refs=0, chroma_me=0, weightb=0)
SUPERFAST = dict(me_method=0, subme=1, rd=0, trellis=0, psy_rd_q8=0, partitions=6, refs=1, mixed_refs=0, chroma_me=0)


@pytest.mark.parametrize("case,over,types", [("ultrafast", ULTRAFAST, "IPPPPP"), ("superfast", SUPERFAST, "IBBPBP")])
def test_device_abi_stream_decodes_on_the_checker(gpu, case, over, types):
    from test_gpu_b_pred_reuse import static_frames
    w, h = 96, 80
    frames = [static_frames(w, h, len(types), 40 + s, 4) for s in range(2)]
    s = AnySession(gpu, w, h, **over)
    pics = s.code(frames, types, update=600, write=True)
    off = s.offsets()
    s.close()
    assert off[0].any() and off[1].any() and not np.array_equal(off[0], off[1]), "every stream its own state"
    dec = O.h264_decode(s.stream, len(types), w, h)
    assert len(dec) == len(types)
    for k, p in enumerate(pics):
        assert np.array_equal(dec[k], p["recon"][0]), f"{case}: picture {k} of the device's stream decodes differently"


# ---- (6) refusals on the device ----
def _set_any(gpu, cfg):
    import torch
    from gpu_enc import GpuEncoder
    gg = GpuEncoder(cfg)
    d_off, d_pic = torch.zeros(192, dtype=torch.int16, device="cuda"), torch.zeros(1552, dtype=torch.uint8, device="cuda")
    rc = gpu.x264gpu_encoder_set_nr_any(gg.h, d_off.data_ptr(), d_pic.data_ptr())
    back = gpu.x264gpu_encoder_set_nr_any(gg.h, None, None)
    half = gpu.x264gpu_encoder_set_nr_any(gg.h, d_off.data_ptr(), None)
    gg.close()
    return rc, back, half


@pytest.mark.parametrize("why,over", [("dpb == 0", dict(dpb=0, weightb=0, me_method=0)), ("psy-trellis", dict(psy_trellis_q8=256, me_method=1)),
                                      ("qp_rd", dict(qp_rd=1, subme=10, rd=63 | 64, trellis=127, me_method=1, aq_mode=1))])
def test_set_nr_any_refuses(gpu, why, over):
    rc, back, half = _set_any(gpu, O.default_config(W, H, streams=1, **dict(G.MEDIUM, **over)))
    assert rc == -1, f"{why}: EINVAL"
    assert back == 0 and half == -1, "NULL, NULL returns to the plain kernels; one pointer alone is EINVAL"


def test_set_nr_any_admits_what_set_nr_refuses(gpu):
    for over in (dict(cabac=0, trellis=0), dict(me_method=0), dict(NORD, me_method=3, me_range=8)):
        rc, back, _ = _set_any(gpu, O.default_config(W, H, streams=1, **dict(G.MEDIUM, **over)))
        assert rc == 0 and back == 0, over


# ---- (7) host sessions of the fast presets, each in a process of its own ----
def _child(tmp_path, preset, tune, nr, env, *extra):
    e = dict(os.environ)
    e.pop("X264GPU_NR_ANY", None)
    e.update(env)
    r = subprocess.run([sys.executable, os.path.join(HERE, "nr_any_child.py"), str(tmp_path), preset, tune, str(nr), *extra], capture_output=True, text=True, timeout=300, env=e)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


@pytest.mark.parametrize("preset,tune", [("ultrafast", "-"), ("superfast", "-"), ("veryfast", "-"), ("faster", "-"), ("medium", "zerolatency")])
def test_host_session_of_a_fast_preset(gpu, tmp_path, preset, tune):
    out = _child(tmp_path, preset, tune, 200, {"X264GPU_NR_ANY": "1"})
    print(f"{preset} {tune}: non-zero inter levels nr 200 {out['levels_nr']} / nr 0 {out['levels_plain']}; coded inter macroblocks {out['inter_nr']} / {out['inter_plain']}; bframes {out['bframes']} cabac {out['cabac']}")
    assert out["nr"] == 200 and not G._nr_warnings(out["log"]), out["log"]
    assert sum("runs on the extended toolset" in t for _, t in out["log"]) == 1, out["log"]
    assert out["plain_nr"] == 0
    assert out["decoded"] and out["plain_decoded"], "the stream decodes on the checker to the session's reconstruction"
    assert out["same"], "a second run gives other bytes"
    assert out["inter_plain"] > 0 and out["levels_nr"] < out["levels_plain"], (out["levels_nr"], out["levels_plain"])


def test_without_the_variable_ultrafast_reports_nr_0(gpu, tmp_path):
    out = _child(tmp_path, "ultrafast", "-", 200, {}, "open")
    w = G._nr_warnings(out["log"])
    assert out["nr"] == 0 and len(w) == 1 and "needs CABAC" in w[0] and w[0].rstrip().endswith("nr 0"), out["log"]


# ---- (8) batching: one group per strength ----
VERYFAST = dict(G.BATCH, me="hex", subme=2, trellis=0, ref=1)
del VERYFAST["qp"]
VERYFAST["crf"] = 24


def test_batched_sessions_code_what_they_code_alone(gpu):
    from test_gpu_b_pred_reuse import static_frames
    from test_gpu_quality import _with_env
    nrs = [600, 150, 600, 150]
    frames_of = [static_frames(96, 80, 6, 60 + i, 12) for i in range(4)]          # (noise a veryfast-like CRF session does not skip: the offsets must move)
    opts_of = [dict(VERYFAST, nr=nr) for nr in nrs]
    solo = _with_env({"X264GPU_NR_ANY": "1"}, lambda: [G._host(o, f) for o, f in zip(opts_of, frames_of)])
    res, errs = [None] * 4, []

    def one(i):
        try:
            res[i] = G._host(opts_of[i], frames_of[i], recon=False)
        except BaseException as e:  # noqa: BLE001
            errs.append(f"session {i}: {e!r}")
    ths = [threading.Thread(target=one, args=(i,)) for i in range(4)]
    _with_env({"X264GPU_NR_ANY": "1", "X264GPU_BATCH": "2"}, lambda: ([t.start() for t in ths], [t.join() for t in ths]))
    assert not errs, errs
    for i in range(4):
        a, b = res[i], solo[i]
        assert a["nr"] == b["nr"] == nrs[i] and not G._nr_warnings(a["log"]) and not G._nr_warnings(b["log"]), (i, a["log"])
        assert any("X264GPU_BATCH: stream" in t for _, t in a["log"]), "the session ran in a batch group"
        assert a["stream"] == b["stream"] and len(a["stream"]) > 0, f"session {i} (nr {nrs[i]}) codes other bytes in its group than alone"
        assert np.array_equal(a["offs"][-1], b["offs"][-1]) and a["offs"][-1].any(), i

"""-m gpu: x264's QP-RD (--subme 10; cfg.qp_rd) on the device.
(1) the walk as a primitive (x264gpu_qprd_walk: the state machine of csrc/qprd.hip.h over tables) against its Python twin (tests/qprd_ref.py, pinned on hand-worked cases
by tests/test_qprd_cpu.py); (2) a QP-RD session whose range is the single quantiser of its pictures must equal the session without QP-RD byte for byte — the extra
candidate passes disturb nothing of the decided macroblock; (3) the walk inside the macroblock loop, from the log the QPRD instantiations write: replayed through the
twin, the chosen quantiser in the records, the stream decodable to the device's reconstruction; (4) whole sessions through x264_encoder_encode."""
import ctypes as C
import functools

import numpy as np
import pytest

import bgop
import oracle_lib as O
import qprd_ref as R
from synth import synth_frames
from test_gpu_bframes import MEDIUM

pytestmark = pytest.mark.gpu

W, H = 64, 48          # 4 x 3 macroblocks: the interior ones have every neighbour
NMB = 12
TOOL = dict(MEDIUM, subme=9, rd=63 | 64, trellis=127)          # x264 --subme 9 --trellis 2: what QP-RD stands on (the refinement instantiations, RD 6)
TYPES = "IBBBP"        # coding order I P Bref b b
MB_I16x16 = 2          # X264GPU_MB_I16x16


# ---- (1) the primitive ----
def _problems(rng, n, lo, hi):
    """costs from few distinct values (ties), cbp_empty runs at the high-qp end, last_qp anywhere in the range"""
    cost = rng.integers(90, 100, (n, 52)).astype(np.int32)
    slope = rng.integers(-3, 4, (n, 1))
    cost += (slope * (np.arange(52)[None, :] - rng.integers(lo, hi + 1, (n, 1)))).clip(-40, 40).astype(np.int32) // 2
    flip = (cost + rng.integers(-2, 3, (n, 52))).astype(np.int32)
    first_empty = rng.integers(lo - 2, hi + 6, (n, 1))          # from here up nothing is coded (below lo: everywhere; above hi: nowhere)
    empty = (np.arange(52)[None, :] >= first_empty).astype(np.uint8)
    orig = rng.integers(lo, hi + 1, n).astype(np.int32)
    near = np.clip(orig + rng.integers(-3, 4, n), lo, hi)
    last = np.where(rng.random(n) < 0.6, near, rng.integers(lo, hi + 1, n)).astype(np.int32)
    t8 = rng.integers(0, 2, n).astype(np.int32)
    return cost, empty, flip, orig, last, t8


@pytest.mark.parametrize("lo,hi", [(1, 51), (20, 30), (26, 26)])
@pytest.mark.parametrize("psy", [0, 1])
def test_primitive_equals_twin(gpu, psy, lo, hi):
    import torch
    lib = gpu
    n = 256
    cost, empty, flip, orig, last, t8 = _problems(np.random.default_rng(1000 * psy + lo), n, lo, hi)
    dev = [torch.from_numpy(a).cuda() for a in (cost, empty, flip, orig, last, t8)]
    d_qp, d_flip, d_n = (torch.zeros(n, dtype=torch.int32, device="cuda") for _ in range(3))
    d_asked = torch.full((n, lib.QPRD_ASKED_MAX), -1, dtype=torch.int32, device="cuda")
    lib.check(lib.x264gpu_qprd_walk(*[d.data_ptr() for d in dev], n, lo, hi, psy, d_qp.data_ptr(), d_flip.data_ptr(), d_asked.data_ptr(), d_n.data_ptr(), None), "qprd_walk")
    torch.cuda.synchronize()
    g_qp, g_flip, g_n, g_asked = d_qp.cpu().numpy(), d_flip.cpu().numpy(), d_n.cpu().numpy(), d_asked.cpu().numpy()
    moved = flips = ties = 0
    for p in range(n):
        qp, fl, asked = R.walk(R.table_cost(cost[p], empty[p], flip[p]), int(orig[p]), int(last[p]), lo, hi, psy, bool(t8[p]))
        want = [q | (256 if f else 0) for q, f in asked]
        assert g_n[p] == len(want) <= lib.QPRD_ASKED_MAX and g_asked[p, :g_n[p]].tolist() == want, (p, g_asked[p, :g_n[p]].tolist(), want)
        assert (g_qp[p], g_flip[p]) == (qp, int(fl)), (p, g_qp[p], g_flip[p], qp, fl)
        moved += qp != orig[p]; flips += fl; ties += len({int(cost[p][q]) for q, _ in asked}) < len({q for q, _ in asked})
    if lo < hi:
        assert moved >= n // 8 and flips >= 4 and ties >= n // 8, (moved, flips, ties)          # the problems reach what they are drawn for
    else:
        assert moved == 0 and flips == 0


# ---- the macroblock loop ----
def _frames(streams):
    """per stream its own content: moving texture (tests/synth.py) with a per-stream seed"""
    per = [synth_frames(W, H, len(TYPES), seed=31 + 5 * s) for s in range(streams)]
    return [[per[s][d] for s in range(streams)] for d in range(len(TYPES))]          # [display index][stream]


OFFSETS = (0, 4, -4, 0, -2, 3, 0, -4, 4, 1, 0, -1)


def _offsets(streams, nmb):
    """quantiser offsets that swing by up to +-4 from macroblock to macroblock (some macroblocks stay at the picture's quantiser: with every macroblock pushed
    away from it, every walk comes back and none keeps its quantiser), per stream a rotation of their own; 0 at every stream's first macroblock (the slice's quantiser)"""
    off = np.zeros((streams, nmb), np.float32)
    for s in range(streams):
        for i in range(1, nmb):
            off[s, i] = OFFSETS[(i + 5 * s) % len(OFFSETS)]
    return off


def _run(gpu, me, qp_rd, qps, offsets=None, qp_range=(0, 0), log=False, types=TYPES, streams=2):
    """-> per coding position: (picture type, records [S][nmb], levels, [recon per stream], log [S][nmb][words] or None), and the streams' bytes"""
    import torch
    from gpu_enc import GpuEncoder
    from x264vfw_amd import host_api as HL
    lib = gpu
    kw = dict(TOOL, me_method=me, qp_rd=qp_rd, qp_min=qp_range[0], qp_max=qp_range[1])
    cfg = O.default_config(W, H, streams=streams, **kw)
    gg = GpuEncoder(cfg)
    keep = []
    if offsets is not None:
        d_off = torch.from_numpy(offsets).cuda(); keep.append(d_off)
        lib.check(lib.x264gpu_encoder_set_mb_qp_offsets(gg.h, d_off.data_ptr()), "set_mb_qp_offsets")
    d_log = None
    if log:
        d_log = torch.zeros((streams, gg.n, lib.QPRD_LOG_WORDS), dtype=torch.int32, device="cuda")
        lib.check(lib.x264gpu_encoder_set_qprd_log(gg.h, d_log.data_ptr()), "set_qprd_log")
    frames = _frames(streams)
    dpb = bgop.HostDpb(HL, kw["refs"], 3, 1)
    order = bgop.schedule(types, 1)
    hdr = dpb.headers(W, H, qps[1], cfg.chroma_qp_offset, kw["refs"], cfg.dct8x8, cfg.weightb)
    bytes_ = [hdr] * streams
    out = []
    for k, (disp, pt) in enumerate(order):
        pic, _ = dpb.plan(pt, disp, bgop.follow_of(order, k))
        pic.qp = bgop.pic_qp(pt, *qps)
        if d_log is not None:
            d_log.fill_(-1)
        mbs, lvs = gg.encode_pics(frames[disp], [pic] * streams)
        recs = [gg.recon(s) for s in range(streams)]
        for s in range(streams):
            bytes_[s] += dpb.slice(W // 16, H // 16, pic.qp, qps[1], 0, 0, kw["refs"], cfg.dct8x8, mbs[s], lvs[s])
        out.append((pt, pic.qp, mbs.copy(), lvs.copy(), recs, None if d_log is None else d_log.cpu().numpy().view(np.uint32).copy()))
        dpb.commit()
    gg.close()
    return out, bytes_


# ---- (2) a range of one quantiser: nothing may change ----
@pytest.mark.parametrize("me", [1, 2])
def test_single_quantiser_range_equals_no_qprd(gpu, me):
    qp = 24
    zero = np.zeros((2, NMB), np.float32)
    a, _ = _run(gpu, me, 0, (qp, qp, qp), offsets=zero)
    b, _ = _run(gpu, me, 1, (qp, qp, qp), offsets=zero, qp_range=(qp, qp), log=True)
    assert [p[0] for p in a] == [0, 2, 3, 4, 4]          # I, P, B reference, b, b
    walked = 0
    for k, (pa, pb) in enumerate(zip(a, b)):
        assert np.array_equal(pa[2].view(np.uint8), pb[2].view(np.uint8)), f"picture {k} (type {pa[0]}): records differ"
        assert np.array_equal(pa[3], pb[3]), f"picture {k} (type {pa[0]}): levels differ"
        for s in range(2):
            assert np.array_equal(pa[4][s], pb[4][s]), f"picture {k} (type {pa[0]}) stream {s}: reconstruction differs"
        walked += int((pb[5][:, :, 0] > 0).sum())
    assert walked >= 5 * NMB, "the QP-RD instantiations ran their walks (the log says so)"
    assert not np.array_equal(a[1][2][0].view(np.uint8), a[1][2][1].view(np.uint8)), "the two streams differ"


# ---- (3) the walk in the loop ----
def _entry(words):
    n = int(words[0])
    assert 0 <= n <= 63
    h = int(words[1])
    samples = [(int(words[2 + 2 * i]) & 255, bool(int(words[2 + 2 * i]) >> 8 & 1), bool(int(words[2 + 2 * i]) >> 16 & 1), int(np.int32(words[3 + 2 * i]))) for i in range(n)]
    return n, (h & 255, h >> 8 & 255, h >> 16 & 255, h >> 24 & 1), samples


def _replay(samples, orig, last, lo, hi, psy, t8):
    """the twin over the logged samples: every encode it asks for must be the next one logged"""
    it = iter(samples)

    def cost(q, flip):
        sq, se, sf, sc = next(it)
        assert (sq, sf) == (q, flip), f"the twin asks for {(q, flip)}, the device coded {(sq, sf)}"
        return sc, se
    qp, fl, asked = R.walk(cost, orig, last, lo, hi, psy, t8)
    assert next(it, None) is None, "the device coded more than the twin asks for"
    return qp, fl


def _check_logged_picture(pt, qp_pic, mbs, log, offsets, t8_cfg, kept_moved):
    for s in range(mbs.shape[0]):
        kept = moved = 0
        for i in range(mbs.shape[1]):
            n, (orig, last, chosen, flip), samples = _entry(log[s, i])
            m = mbs[s][i]
            t, coded = int(m["type"]), bool(m["cbp_luma"]) or bool(m["cbp_chroma"])
            if n == 0:
                assert t in (O.MB_P_SKIP, O.MB_B_SKIP), f"type {pt} stream {s} macroblock {i}: no walk in a macroblock of type {t}"
                continue
            inter = t >= O.MB_P_L0
            assert samples[0][0] == orig and not samples[0][2]
            # (the transform size may be chosen in every inter macroblock of a --8x8dct session; whether the device thought so shows in the replay)
            qp, fl = _replay(samples, orig, last, 1, 51, True, inter and t8_cfg)
            assert (qp, int(fl)) == (chosen, flip), f"type {pt} stream {s} macroblock {i}: twin {(qp, fl)}, device {(chosen, flip)}"
            # x264's strictly-less rule, said another way: the FIRST of the cheapest compared encodes wins (the jump down of a macroblock with nothing coded is not compared)
            cmp_ = [(c, k) for k, (q, e, f, c) in enumerate(samples) if not f and not (k == 1 and samples[0][1])]
            assert samples[min(cmp_)[1]][0] == chosen
            # the record: the chosen quantiser, unless nothing is coded — then the previous one's (an Intra_16x16 without levels never raises it)
            dc16 = t == MB_I16x16 and bool(int(m["nnz"]) >> 24 & 1)
            want = chosen if coded or dc16 else min(chosen, last) if t == MB_I16x16 else last
            assert int(m["qp"]) == want, f"type {pt} stream {s} macroblock {i}: record.qp {int(m['qp'])}, chosen {chosen}, last {last}, coded {coded}"
            kept += chosen == orig; moved += chosen != orig
        kept_moved.append((pt, s, kept, moved))


@functools.lru_cache(maxsize=None)
def _walk_runs(me):
    from x264vfw_amd import lib
    off = _offsets(2, NMB)
    return _run(lib, me, 1, (22, 24, 26), offsets=off, log=True), off


@pytest.mark.parametrize("me", [1, 2])
def test_walk_in_the_loop_replays_through_the_twin(gpu, me):
    (pics, bytes_), off = _walk_runs(me)
    km = []
    ups = downs = 0
    for pt, qp_pic, mbs, lvs, recs, log in pics:
        _check_logged_picture(pt, qp_pic, mbs, log, off, True, km)
        for s in range(2):
            for i in range(NMB):
                n, (orig, last, chosen, flip), _ = _entry(log[s, i])
                ups += n > 0 and last > orig; downs += n > 0 and last < orig
    assert ups >= 10 and downs >= 10, (ups, downs)          # last_qp != orig_qp in both directions
    for pt, s, kept, moved in km:
        assert kept >= 1 and moved >= 1, f"picture type {pt} stream {s}: {kept} macroblocks keep their quantiser, {moved} leave it"
    # the quantisers the walks chose are what the macroblocks were coded with: the streams decode to the device's reconstructions
    for s in range(2):
        dec = O.h264_decode(bytes_[s], len(pics), W, H)
        for k, d in enumerate(dec):
            assert np.array_equal(d, pics[k][4][s]), f"stream {s}: picture {k} decodes differently"


def test_first_macroblocks_that_keep_their_quantiser_equal_no_qprd(gpu):
    """the 16 x 128 picture of one slice per macroblock row (tests/test_gpu_psy_trellis.py): every macroblock is the first of its slice, so a macroblock whose
    walk ends where it began, without a flip, must be coded exactly as without QP-RD — nothing else can differ"""
    import torch
    from gpu_enc import GpuEncoder
    from test_gpu_psy_trellis import MBH, MBW, QP, first_mb_frames
    lib = gpu
    frames = first_mb_frames()
    got = {}
    for qp_rd in (0, 1):
        cfg = O.default_config(16 * MBW, 16 * MBH, streams=2, qp_i=QP, partitions=7, dct8x8=1, cabac=1, rd=63 | 64, subme=9, psy=1, psy_rd_q8=256, chroma_qp_offset=-2,
                               trellis=127, me_method=1, slices=MBH, slices_plain=1, qp_rd=qp_rd)
        gg = GpuEncoder(cfg)
        d_log = torch.full((2, gg.n, lib.QPRD_LOG_WORDS), -1, dtype=torch.int32, device="cuda")
        if qp_rd:
            lib.check(lib.x264gpu_encoder_set_qprd_log(gg.h, d_log.data_ptr()), "set_qprd_log")
        mbs, lvs = gg.encode(frames, O.SLICE_I)
        got[qp_rd] = (mbs.copy(), lvs.copy(), d_log.cpu().numpy().view(np.uint32))
        gg.close()
    kept = moved = 0
    for s in range(2):
        for m in range(MBH):
            n, (orig, last, chosen, flip), samples = _entry(got[1][2][s, m])
            assert n >= 2 and orig == last == QP          # the first macroblock of a slice: last_qp is the slice's quantiser, its own
            assert _replay(samples, orig, last, 1, 51, True, False) == (chosen, bool(flip))
            if chosen == orig and not flip:
                kept += 1
                assert got[1][0][s][m].tobytes() == got[0][0][s][m].tobytes(), f"stream {s} macroblock {m}: record differs from the run without QP-RD"
                assert np.array_equal(got[1][1][s][m], got[0][1][s][m]), f"stream {s} macroblock {m}: levels differ from the run without QP-RD"
            else:
                moved += 1
    assert kept >= 2 and moved >= 1, (kept, moved)


# ---- (4) whole sessions through x264_encoder_encode ----
SESSION = {"crf": 26, "me": "umh", "subme": 10, "trellis": 2, "aq-mode": 1, "bframes": 3, "b-adapt": 0, "keyint": 30}
# ... and under --threads 2: GOP slots whose quantisers are planned ahead (X264GPU_GOP_SLOTS_RC=1 admits CRF with B pictures there; the slots need a keyint they fit)
SLOTS = dict(SESSION, threads=2, keyint=4, **{"min-keyint": 4})


def _session(opts, w=64, h=48, n=7):
    """tests/test_gpu_psy_trellis._session's pattern: -> stream, reconstructions and types per picture out, the log, the effective parameters"""
    import host_lib as HL
    from quality_sessions import make_logger
    H = HL.H
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", None) == 0
    p.i_width, p.i_height, p.i_csp = w, h, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for k, v in opts.items():
        assert H.x264_param_parse(C.byref(p), k.encode(), None if v is None else str(v).encode()) == 0, (k, v)
    log = []
    cb = make_logger(log)
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 2
    p.b_vfr_input = 0
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_, "x264_encoder_open failed"
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    stream, recons, types = b"", [], []

    def take(size):
        nonlocal stream
        assert size >= 0
        if size:
            stream += C.string_at(nal[0].p_payload, size)
            rec = np.zeros(w * h * 3 // 2, np.uint8)
            assert H.x264host_get_recon(h_, rec.ctypes.data) == 0 or eff.i_threads > 1          # (GOP slots hand out no reconstruction: their stream is compared with the --threads 1 session's)
            recons.append(rec); types.append(int(out.i_type))
    for i, f in enumerate(synth_frames(w, h, n, seed=11)):
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out)))
    guard = 0
    while H.x264_encoder_delayed_frames(h_) and guard < 4 * n:
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out)))
        guard += 1
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return dict(stream=stream, recons=recons, types=types, log=log, subme=int(eff.analyse.i_subpel_refine), threads=int(eff.i_threads))


@pytest.mark.parametrize("opts,env", [(SESSION, {}), (SLOTS, {"X264GPU_GOP_SLOTS_RC": "1"})], ids=["threads1", "gop-slots"])
def test_sessions_with_qprd(gpu, monkeypatch, opts, env):
    n, w, h = 7, 64, 48
    monkeypatch.setenv("X264GPU_QP_RD", "1")          # (read at every x264_encoder_open)
    for k, v in env.items():
        monkeypatch.setenv(k, v)
    a = _session(opts)
    assert a["subme"] == 10 and a["threads"] == opts.get("threads", 1)
    assert not [m for lvl, m in a["log"] if lvl <= 1], a["log"]          # no warning, no error
    assert len(a["recons"]) == n and 5 in a["types"], f"picture types {a['types']}: the session must hold B pictures"
    serial = a
    if a["threads"] > 1:
        # GOP slots: the pictures of two GOPs side by side in ONE device encoder — byte for byte the --threads 1 session, whose reconstructions can be had
        serial = _session(dict(opts, threads=1))
        assert serial["subme"] == 10 and serial["stream"] == a["stream"] and sorted(serial["types"]) == sorted(a["types"])
    dec = O.h264_decode(serial["stream"], n, w, h)
    assert len(dec) == n
    for i in range(n):
        np.testing.assert_array_equal(dec[i], serial["recons"][i], err_msg=f"decoded picture {i} != encoder reconstruction")
    b = _session(dict(opts, subme=9))
    assert b["subme"] == 9 and b["types"] == a["types"] and b["stream"] != a["stream"]
    # a range of one quantiser leaves QP-RD nothing to choose: the subme 9 stream
    c, d = _session(dict(opts, qpmin=26, qpmax=26)), _session(dict(opts, subme=9, qpmin=26, qpmax=26))
    assert (c["subme"], d["subme"]) == (10, 9) and c["stream"] == d["stream"]
    # without the variable: the subme 9 session, with today's warning
    monkeypatch.delenv("X264GPU_QP_RD")
    e = _session(opts)
    assert e["subme"] == 9 and e["stream"] == b["stream"] and [m for lvl, m in e["log"] if lvl == 1 and "subme 9" in m]


def test_session_qprd_gives_way_to_noise_reduction(gpu, monkeypatch):
    monkeypatch.setenv("X264GPU_QP_RD", "1")
    a = _session(dict(SESSION, nr=100), n=5)
    assert a["subme"] == 9 and [m for lvl, m in a["log"] if lvl == 2 and "QP-RD is not run beside noise reduction" in m], a["log"]

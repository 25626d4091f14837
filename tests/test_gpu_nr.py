"""-m gpu: noise reduction (--nr) on the device against its pure-Python twin (tests/nr_ref.py): the primitive and the state update, the denoising instantiations
of the macroblock loop (zero offsets = the plain kernels, statistics = the twin's, every final-encode site per category, exact re-issue, refusals), and whole
sessions through the device ABI and through x264_encoder_encode decoded by the checker."""
import ctypes as C

import numpy as np
import pytest

import bgop
import nr_ref as N
import oracle_lib as O
from synth import synth_frames

pytestmark = pytest.mark.gpu

MEDIUM = dict(refs=3, dpb=4, weightb=1, partitions=7, dct8x8=1, chroma_me=1, mixed_refs=1, cabac=1, rd=1, subme=7, psy=1, psy_rd_q8=256, chroma_qp_offset=-2, trellis=63)
RD6 = dict(subme=9, rd=63, trellis=127)          # RD refinement + --trellis 2: the <.., 6, ..> instantiations of P and B slices
QPS = (20, 23, 25)
LV_CHROMA_AC = 280


# ---- inputs shared with tests/test_nr_cpu.py (no GPU needed to build them) ----
def update_chain(s):
    """six pictures' statistics of stream s: the counts cross 1 << 18 in category 0 (stream 0) / 2 (stream 1) and 1 << 16 in category 1 (both)"""
    rng = np.random.default_rng(900 + s)
    out = []
    for k in range(6):
        pic = N.zero_state()
        pic["count"] = [60000 + 7 * k, 20000 + k, 900] if s == 0 else [1200, 30000 + 3 * k, 70000 + k]
        for cat in range(3):
            for i in range(N.NCOEF[cat]):
                pic["sum"][cat][i] = int(rng.integers(0, 40 * pic["count"][cat] + 1)) if (i + k) % 5 else 0
        out.append(pic)
    return out


def two_streams(w, h, n, seed, patch_last=False):
    """two streams of the project's synthetic pan with different content; patch_last: four macroblocks of the last picture are occluded by vertical stripes (two
    columns black, two white) under noise of +-12 — nothing in the reference looks like them, the macroblock above does: intra macroblocks with AC levels to code"""
    out = []
    for s in range(2):
        fr = [f.copy() for f in synth_frames(w, h, n, seed=seed + 17 * s)]
        if patch_last:
            rng = np.random.default_rng(seed + s)
            y = fr[-1][:w * h].reshape(h, w)
            stripes = np.where((np.arange(32) // 2) % 2, 223, 28)[None, :] + rng.integers(-12, 13, (32, 32))
            y[16:48, 16:48] = stripes
        out.append(fr)
    return out


# ---- (1) the primitive and the update ----
def _coefs(cat, nblk, rng):
    """int16 coefficients over the range a transform of 8-bit samples holds (4x4: 36 * 255, 8x8: within int16)"""
    lim = 32767 if cat == 1 else 36 * 255
    c = rng.integers(-lim, lim + 1, (nblk, N.NCOEF[cat])).astype(np.int16)
    c[rng.random(c.shape) < 0.3] = 0
    return c


def _offsets(kind, rng):
    off = N.zero_offsets()
    if kind == "random":
        off[:] = rng.integers(0, 3000, (3, 64))
    elif kind == "max":
        off[:] = 32767
    if kind != "zero":
        off[:, 0] = 0
    off[0, 16:] = 0; off[2, 16:] = 0
    return off


@pytest.mark.parametrize("kind", ["random", "zero", "max"])
@pytest.mark.parametrize("cat", [0, 1, 2])
def test_primitive_equals_twin(gpu, cat, kind):
    import torch
    rng = np.random.default_rng(50 + 10 * cat + len(kind))
    nblk = 6 if cat == 1 else 13          # a full pass of the kernel's layout and a partial one (8x8: four blocks a pass) / one partial pass of sixteen
    for nb in (nblk, 21 if cat != 1 else 4):
        coefs, off = _coefs(cat, nb, rng), _offsets(kind, rng)
        want, sums = N.denoise_blocks(coefs, cat, off)
        d_c, d_o = torch.from_numpy(coefs.copy()).cuda(), torch.from_numpy(off.copy().view(np.int16)).cuda()
        d_s = torch.full((1552,), 0xAB, dtype=torch.uint8, device="cuda")
        gpu.check(gpu.x264gpu_denoise_blocks(d_c.data_ptr(), nb, cat, d_o.data_ptr(), d_s.data_ptr(), None), "denoise_blocks")
        torch.cuda.synchronize()
        np.testing.assert_array_equal(d_c.cpu().numpy(), want)
        got = d_s.cpu().numpy().tobytes()
        assert N.sums_from_bytes(got) == sums and got[:1548] == N.sums_struct(sums)[:1548]
        assert np.array_equal(d_o.cpu().numpy().view(np.uint16), off), "the offsets are read only"


def test_update_equals_twin_over_a_chain(gpu):
    import torch
    strength = 600
    d_off = torch.full((2, 192), 0x5a5a, dtype=torch.int16, device="cuda")
    d_state = torch.zeros((2, 1552), dtype=torch.uint8, device="cuda")
    chains, states = [update_chain(0), update_chain(1)], [N.zero_state(), N.zero_state()]
    for k in range(6):
        pics = b"".join(N.sums_struct(chains[s][k]) for s in range(2))
        d_pic = torch.from_numpy(np.frombuffer(pics, np.uint8).copy()).cuda()
        gpu.check(gpu.x264gpu_nr_update(d_off.data_ptr(), d_state.data_ptr(), d_pic.data_ptr(), 2, strength, None), "nr_update")
        torch.cuda.synchronize()
        off, st = d_off.cpu().numpy().view(np.uint16).reshape(2, 3, 64), d_state.cpu().numpy()
        for s in range(2):
            want = N.update(states[s], chains[s][k], strength)
            np.testing.assert_array_equal(off[s], want, err_msg=f"picture {k} stream {s}")
            assert N.sums_from_bytes(st[s].tobytes()) == states[s], f"picture {k} stream {s}: state"
    # d_pic NULL: offsets from the state as it is, at another strength
    gpu.check(gpu.x264gpu_nr_update(d_off.data_ptr(), d_state.data_ptr(), None, 2, 77, None), "nr_update")
    torch.cuda.synchronize()
    off = d_off.cpu().numpy().view(np.uint16).reshape(2, 3, 64)
    for s in range(2):
        np.testing.assert_array_equal(off[s], N.update(states[s], None, 77))


# ---- sessions through the device ABI ----
class Session:
    """two streams through x264gpu_encode_pictures, planned by the product's DPB model; nr: set_nr with offsets (None: the plain session)"""

    def __init__(self, lib, w, h, offsets=None, nr=True, **over):
        import torch
        from gpu_enc import GpuEncoder
        from x264vfw_amd import host_api as HL
        self.lib, self.t, self.w, self.h = lib, torch, w, h
        self.kw = dict(MEDIUM, **over)
        self.cfg = O.default_config(w, h, streams=2, **self.kw)
        self.gg = GpuEncoder(self.cfg)
        self.dpb = bgop.HostDpb(HL, self.kw["refs"], 3, 1, weightp=0)
        self.stream = self.dpb.headers(w, h, QPS[1], self.cfg.chroma_qp_offset, self.kw["refs"], self.cfg.dct8x8, self.cfg.weightb)
        self.nr = nr
        self.d_off = torch.zeros((2, 192), dtype=torch.int16, device="cuda")
        self.d_pic = torch.full((2, 1552), 0xCD, dtype=torch.uint8, device="cuda")
        self.d_state = torch.zeros((2, 1552), dtype=torch.uint8, device="cuda")
        if offsets is not None:
            self.set_offsets(offsets)
        if nr:
            lib.check(lib.x264gpu_encoder_set_nr(self.gg.h, self.d_off.data_ptr(), self.d_pic.data_ptr()), "set_nr")

    def set_offsets(self, off):
        self.d_off.copy_(self.t.from_numpy(np.ascontiguousarray(np.broadcast_to(off, (2, 3, 64)), np.uint16).view(np.int16).reshape(2, 192)))
        self.t.cuda.synchronize()

    def offsets(self):
        return self.d_off.cpu().numpy().view(np.uint16).reshape(2, 3, 64)

    def pic_sums(self):
        raw = self.d_pic.cpu().numpy()
        return [N.sums_from_bytes(raw[s].tobytes()) for s in range(2)]

    def update(self, strength):
        self.lib.check(self.lib.x264gpu_nr_update(self.d_off.data_ptr(), self.d_state.data_ptr(), self.d_pic.data_ptr(), 2, strength, None), "nr_update")
        self.t.cuda.synchronize()

    def code(self, frames, types, update=None, write=False):
        """frames[s][display index]; -> per coded picture dict(pt, disp, mb, lv, recon[2], sums[2])"""
        order = bgop.schedule(types, 1)
        mbw, mbh = (self.w + 15) // 16, (self.h + 15) // 16
        out = []
        for k, (disp, pt) in enumerate(order):
            pic, _ = self.dpb.plan(pt, disp, bgop.follow_of(order, k))
            pic.qp = bgop.pic_qp(pt, *QPS)
            mb, lv = self.gg.encode_pics([frames[0][disp], frames[1][disp]], [pic, pic])
            rec = dict(pt=pt, disp=disp, pic=pic, mb=mb.copy(), lv=lv.copy(), recon=[self.gg.recon(0), self.gg.recon(1)], sums=self.pic_sums() if self.nr else None)
            if write:
                self.stream += self.dpb.slice(mbw, mbh, pic.qp, QPS[1], 0, 0, self.kw["refs"], self.cfg.dct8x8, mb[0], lv[0],
                                              slices=(-self.cfg.slices if self.cfg.slices_plain else self.cfg.slices) if self.cfg.slices > 1 else 1)
            if update is not None and self.nr:
                self.update(update)
            self.dpb.commit()
            out.append(rec)
        return out

    def close(self):
        self.gg.close()
        self.dpb.close()


def _same_pictures(a, b, what):
    assert len(a) == len(b)
    for k, (x, y) in enumerate(zip(a, b)):
        assert x["mb"].tobytes() == y["mb"].tobytes(), f"{what}: records of picture {k} differ"
        assert x["lv"].tobytes() == y["lv"].tobytes(), f"{what}: levels of picture {k} differ"
        for s in range(2):
            assert np.array_equal(x["recon"][s], y["recon"][s]), f"{what}: reconstruction of picture {k}, stream {s} differs"


# ---- (2) zero offsets are the plain kernels ----
@pytest.mark.parametrize("me", [1, 2])
@pytest.mark.parametrize("level", ["rd3", "rd6"])
def test_zero_offsets_are_the_plain_kernels(gpu, me, level):
    w, h = 96, 80
    frames = two_streams(w, h, 5, 31)
    over = dict(me_method=me, slices=2, slices_plain=1, **(RD6 if level == "rd6" else {}))
    runs = []
    for nr in (False, True):
        s = Session(gpu, w, h, nr=nr, **over)
        runs.append(s.code(frames, "IPBBP"))
        if nr:
            assert not s.offsets().any()
        s.close()
    _same_pictures(runs[0], runs[1], f"me {me} {level}")
    assert any(p["sums"][s]["count"][c] for p in runs[1] for s in range(2) for c in range(3)), "the denoising kernels ran: some statistics"
    assert all(not any(p["sums"][s]["count"]) for p in runs[1] if p["pt"] <= 1 for s in range(2)), "an I picture has none"


# ---- (3) statistics equal the twin's ----
@pytest.mark.parametrize("slices", [1, 3])
def test_statistics_equal_twin(gpu, slices):
    w, h = 96, 80
    frames = two_streams(w, h, 3, 31)
    over = dict(refs=1, slices=slices, slices_plain=1) if slices > 1 else dict(refs=1)
    s = Session(gpu, w, h, **over)
    pics = s.code(frames, "IPP", update=300)
    s.close()
    seen = set()
    for k in (1, 2):
        for st in range(2):
            mbs = pics[k]["mb"][st]
            for m in mbs:
                t = int(m["type"])
                seen.add("skip" if t == O.MB_P_SKIP else "intra" if t < O.MB_P_L0 else ("p16" if int(m["partition"]) == 0 else "split") )
                if t in (O.MB_P_L0, O.MB_P_8x8):
                    seen.add("t8" if m["transform8x8"] else "t4")
            want = N.picture_sums(O, frames[st][pics[k]["disp"]], pics[k - 1]["recon"][st], mbs, w, h)
            got = pics[k]["sums"][st]
            assert got["count"] == want["count"], f"picture {k} stream {st}: counts {got['count']} twin {want['count']}"
            assert got["sum"] == want["sum"], f"picture {k} stream {st}: sums differ"
    assert {"p16", "split", "t8", "t4", "skip"} <= seen, f"the pictures must hold every kind of macroblock: {seen}"


# ---- (4) every final-encode site denoises, per category ----
def _inter_ok(m, lv, cats):
    """the levels of one inter macroblock under offsets of 32767 in the categories `cats`: (holds, non-zero AC levels of the categories not in cats)"""
    luma, cac = lv[:256].reshape(16, 16), lv[LV_CHROMA_AC:LV_CHROMA_AC + 128]
    t8 = bool(m["transform8x8"])
    ok, other = True, 0
    if t8:
        ac = luma.copy(); ac[0::4, 0] = 0          # an 8x8 block's level 0 of the zigzag sits at entry 0 of its first 4x4 block
    else:
        ac = luma.copy(); ac[:, 0] = 0
    if (1 if t8 else 0) in cats: ok = ok and not ac.any()
    else: other += int(np.count_nonzero(ac))
    if 2 in cats: ok = ok and not cac.any()
    else: other += int(np.count_nonzero(cac))
    return ok, other


@pytest.mark.parametrize("cats", [(0, 1, 2), (0,), (1,), (2,)])
def test_every_final_encode_site_denoises(gpu, cats):
    w, h = 96, 80
    frames = two_streams(w, h, 5, 31, patch_last=True)
    off = N.zero_offsets()
    for c in cats:
        off[c, 1:N.NCOEF[c]] = 32767
    s = Session(gpu, w, h, offsets=off)
    pics = s.code(frames, "IPBBP")
    s.close()
    ninter = nintra_ac = other = 0
    kinds = set()
    for p in pics:
        if p["pt"] <= 1:
            continue
        for st in range(2):
            for m, lv in zip(p["mb"][st], p["lv"][st]):
                t = int(m["type"])
                if t in (O.MB_P_SKIP, O.MB_B_SKIP):
                    assert not lv.any()
                elif t >= O.MB_P_L0:
                    ok, o = _inter_ok(m, lv, cats)
                    assert ok, f"picture type {p['pt']} macroblock type {t}: AC levels survive offsets of 32767 in categories {cats}: {lv[:256].tolist()} {lv[LV_CHROMA_AC:].tolist()}"
                    ninter += 1; other += o; kinds.add((p["pt"] >= 3, t))
                else:
                    ac = lv[:256].reshape(16, 16).copy()
                    if not m["transform8x8"]: ac[:, 0] = 0
                    else: ac[0::4, 0] = 0
                    nintra_ac += int(ac.any() or lv[LV_CHROMA_AC:LV_CHROMA_AC + 128].any())
    assert ninter > 20 and any(b for b, _ in kinds) and any(not b for b, _ in kinds), f"inter macroblocks of P and of B pictures: {ninter} {kinds}"
    assert nintra_ac >= 1, "an intra macroblock with AC levels (the occluding patch): intra blocks are not denoised"
    if len(cats) < 3:
        assert other >= 1, f"categories other than {cats} keep AC levels somewhere"


# ---- (5) re-issue is exact ----
def test_reissue_is_exact(gpu):
    import torch
    w, h = 64, 48
    frames = two_streams(w, h, 2, 31)
    rng = np.random.default_rng(5)
    off = _offsets("random", rng)
    off[:] //= 30          # (offsets a real session reaches: most levels survive)
    s = Session(gpu, w, h, offsets=off)
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


# ---- (6) the checker decodes what is coded, on both paths; (7) it is felt and reported; (8) determinism ----
def test_device_abi_stream_decodes_on_the_checker(gpu):
    from test_gpu_b_pred_reuse import static_frames
    w, h, types = 96, 80, "IBBPBP"
    frames = [static_frames(w, h, len(types), 40 + s, 4) for s in range(2)]
    s = Session(gpu, w, h)
    pics = s.code(frames, types, update=600, write=True)
    off = s.offsets()
    s.close()
    assert off[0].any() and off[1].any() and not np.array_equal(off[0], off[1]), "every stream its own state"
    dec = O.h264_decode(s.stream, len(types), w, h)
    assert len(dec) == len(types)
    for k, p in enumerate(pics):
        assert np.array_equal(dec[k], p["recon"][0]), f"picture {k} of the device's stream decodes differently"


def _host(opts, frames, w=96, h=80, recon=True):
    """one session through x264_encoder_encode (frames None: opened and closed only); -> dict(stream, recons, types, log, offsets after every picture, and what
    x264_encoder_parameters reports: nr, psy_trellis, cqo)"""
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
    p.pf_log, p.i_log_level = C.cast(cb, C.c_void_p).value, 3
    p.b_vfr_input = 0
    p.b_annexb, p.b_repeat_headers = 1, 1
    h_ = H.x264_encoder_open_157(C.byref(p))
    assert h_, "x264_encoder_open failed"
    eff = HL.Param()
    H.x264_encoder_parameters(h_, C.byref(eff))
    pic, out = HL.Picture(), HL.Picture()
    assert H.x264_picture_alloc(C.byref(pic), HL.X264_CSP_I420, w, h) == 0
    nal, nn = C.POINTER(HL.Nal)(), C.c_int()
    res = dict(stream=b"", recons=[], types=[], offs=[], log=log, nr=eff.analyse.i_noise_reduction, psy_trellis=eff.analyse.f_psy_trellis, cqo=eff.analyse.i_chroma_qp_offset)
    if frames is None:
        H.x264_encoder_close(h_)
        return res

    def take(size):
        assert size >= 0
        if size:
            res["stream"] += C.string_at(nal[0].p_payload, size)
            rec = np.zeros(w * h * 3 // 2, np.uint8)
            assert not recon or H.x264host_get_recon(h_, rec.ctypes.data) == 0
            o = np.zeros((3, 64), np.uint16)
            H.x264host_nr_offsets(h_, o.ctypes.data)
            res["recons"].append(rec); res["types"].append(int(out.i_type)); res["offs"].append(o)
    for i, f in enumerate(frames):
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out)))
    while H.x264_encoder_delayed_frames(h_):
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out)))
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return res


def _nr_warnings(log):
    return [t for lvl, t in log if lvl <= 1 and "nr (noise reduction)" in t]


def _inter_level_count(pics):
    """non-zero levels of the inter macroblocks of the P and B pictures, both streams"""
    n = 0
    for p in pics:
        if p["pt"] >= 2:
            for st in range(2):
                inter = p["mb"][st]["type"] >= O.MB_P_L0
                n += int(np.count_nonzero(p["lv"][st][inter]))
    return n


HOST = {"qp": 24, "keyint": 30, "bframes": 2, "b-adapt": 0, "me": "hex", "subme": 7, "trellis": 1, "scenecut": 0}


@pytest.fixture(scope="module")
def host_runs():
    from test_gpu_b_pred_reuse import static_frames
    frames = static_frames(96, 80, 6, 40, 4)
    return {nr: _host(dict(HOST, nr=nr), frames) for nr in (600, 0)}, frames


def test_host_session_decodes_on_the_checker(gpu, host_runs):
    runs, frames = host_runs
    a = runs[600]
    assert len(a["recons"]) == 6 and 5 in a["types"], f"picture types {a['types']}: the session must hold B pictures"
    dec = O.h264_decode(a["stream"], 6, 96, 80)
    assert len(dec) == 6
    for i in range(6):
        np.testing.assert_array_equal(dec[i], a["recons"][i], err_msg=f"decoded picture {i} != encoder reconstruction")


def test_it_is_felt_and_reported(gpu, host_runs):
    runs, frames = host_runs
    a, b = runs[600], runs[0]
    assert a["nr"] == 600 and not _nr_warnings(a["log"]), a["log"]
    assert b["nr"] == 0 and not _nr_warnings(b["log"])
    assert not a["offs"][0].any(), "the pictures before the first inter picture leave zero offsets"
    assert a["offs"][1].any() and (a["offs"][1][:, 0] == 0).all(), "offsets after the first P picture"
    assert not any(o.any() for o in b["offs"])


def test_fewer_inter_levels_on_noisy_static_content(gpu):
    """fresh noise of +-4 on a static picture, nr 600 against nr 0 through the device ABI (the state updated behind every picture, as the host does)"""
    from test_gpu_b_pred_reuse import static_frames
    w, h, types = 96, 80, "IBBPBP"
    frames = [static_frames(w, h, len(types), 40 + s, 4) for s in range(2)]
    counts = {}
    for nr in (600, 0):
        s = Session(gpu, w, h, nr=nr > 0)
        counts[nr] = _inter_level_count(s.code(frames, types, update=nr if nr else None))
        s.close()
    print(f"non-zero inter levels over the P and B pictures: nr 600 {counts[600]}, nr 0 {counts[0]}")
    assert counts[600] < counts[0], counts


def test_host_sessions_are_deterministic(gpu, host_runs):
    from test_gpu_b_pred_reuse import static_frames
    runs, frames = host_runs
    again = _host(dict(HOST, nr=600), frames)
    assert again["stream"] == runs[600]["stream"]


def test_vbv_session_codes_a_picture_twice_and_decodes(gpu):
    from test_gpu_b_pred_reuse import static_frames
    frames = static_frames(96, 80, 6, 41, 12)
    opts = dict(HOST, nr=600, crf=18, **{"vbv-maxrate": 60, "vbv-bufsize": 10, "rc-lookahead": 0})
    del opts["qp"]
    a = _host(opts, frames)
    assert a["nr"] == 600 and not _nr_warnings(a["log"])
    assert any("coded again at qp" in t for _, t in a["log"]), "the session must be sized so that a picture is coded twice"
    dec = O.h264_decode(a["stream"], 6, 96, 80)
    assert len(dec) == 6
    for i in range(6):
        np.testing.assert_array_equal(dec[i], a["recons"][i], err_msg=f"decoded picture {i} != encoder reconstruction")
    b = _host(opts, frames)
    assert a["stream"] == b["stream"]


# ---- (9) refusals on the device ----
@pytest.mark.parametrize("over", [dict(cabac=0, trellis=0), dict(me_method=0)])
def test_set_nr_refuses_sessions_without_the_instantiations(gpu, over):
    import torch
    from gpu_enc import GpuEncoder
    gg = GpuEncoder(O.default_config(64, 48, streams=1, **dict(MEDIUM, **over)))
    d_off, d_pic = torch.zeros(192, dtype=torch.int16, device="cuda"), torch.zeros(1552, dtype=torch.uint8, device="cuda")
    assert gpu.x264gpu_encoder_set_nr(gg.h, d_off.data_ptr(), d_pic.data_ptr()) == -1, "EINVAL"
    assert gpu.x264gpu_encoder_set_nr(gg.h, None, None) == 0
    gg.close()


# ---- (10) the host's refusals on the real library: what is missing is named; psy-trellis gives way only to an nr that runs ----
@pytest.mark.parametrize("extra,names", [({"no-cabac": None}, "needs CABAC"), ({"me": "dia"}, "needs me hex / umh"), ({"subme": 5}, "needs subme >= 6"),
                                         ({"trellis": 0}, "needs trellis >= 1"), ({"threads": 4}, "needs threads 1"),
                                         ({"bframes": 0, "weightp": 0}, "needs B-frames, weightp 2 or VBV")])
def test_host_refusals_name_what_is_missing(gpu, extra, names):
    r = _host(dict(HOST, nr=200, **extra), None)
    w = _nr_warnings(r["log"])
    assert r["nr"] == 0 and len(w) == 1 and names in w[0] and w[0].rstrip().endswith("nr 0"), r["log"]


PSY = {"psy-rd": "1.0:0.25"}


def _psy_lines(log):
    return [t for lvl, t in log if lvl <= 1 and "psy-trellis" in t]


@pytest.mark.parametrize("extra", [{"threads": 4}, {"bframes": 0, "weightp": 0}])
def test_a_refused_nr_leaves_psy_trellis_alone(gpu, extra):
    """nr and psy-trellis asked for in a session whose MODE refuses nr: the session reports and runs the psy-trellis (and the chroma quantiser offset) of the same
    session without nr, with the nr warning and no psy-trellis line"""
    a, b = _host(dict(HOST, nr=200, **PSY, **extra), None), _host(dict(HOST, **PSY, **extra), None)
    assert a["nr"] == 0 and len(_nr_warnings(a["log"])) == 1 and not _psy_lines(a["log"]), a["log"]
    assert abs(a["psy_trellis"] - 0.25) < 1e-6 and a["psy_trellis"] == b["psy_trellis"] and a["cqo"] == b["cqo"]


def test_psy_trellis_gives_way_to_an_nr_that_runs(gpu):
    from test_gpu_b_pred_reuse import static_frames
    frames = static_frames(96, 80, 4, 40, 4)
    a, plain, psy = _host(dict(HOST, nr=600, **PSY), frames), _host(dict(HOST, nr=600), frames), _host(dict(HOST, **PSY), None)
    assert a["nr"] == 600 and a["psy_trellis"] == 0 and not _nr_warnings(a["log"]) and len(_psy_lines(a["log"])) == 1, a["log"]
    assert a["cqo"] == plain["cqo"] == psy["cqo"] + 2 and a["stream"] == plain["stream"], "the session is the nr session without psy-trellis, chroma quantiser offset included"


# ---- (11) cross-session batches: every stream of the group its own state; sessions with and without nr, or of different strengths, do not share a group ----
def _batched(n, opts_of, frames_of):
    """len(opts_of) sessions from as many threads under X264GPU_BATCH=n"""
    import threading
    from test_gpu_quality import _with_env
    res, errs = [None] * len(opts_of), []

    def one(i):
        try:
            res[i] = _host(opts_of[i], frames_of[i], recon=False)
        except BaseException as e:  # noqa: BLE001
            errs.append(f"session {i}: {e!r}")
    ths = [threading.Thread(target=one, args=(i,)) for i in range(len(opts_of))]
    _with_env({"X264GPU_BATCH": str(n)}, lambda: ([t.start() for t in ths], [t.join() for t in ths]))
    assert not errs, errs
    return res


BATCH = dict(HOST, keyint=8, **{"min-keyint": 8})


def test_batched_sessions_code_what_they_code_alone(gpu):
    """six sessions under X264GPU_BATCH=2 — two with nr 600, two with nr 150, two without — on different content: three groups, and every session's bytes and
    offsets are those of the same session on its own"""
    from test_gpu_b_pred_reuse import static_frames
    nrs = [600, 150, 0, 600, 0, 150]
    frames_of = [static_frames(96, 80, 6, 60 + i, 4) for i in range(6)]
    opts_of = [dict(BATCH, nr=nr) for nr in nrs]
    solo = [_host(o, f) for o, f in zip(opts_of, frames_of)]
    together = _batched(2, opts_of, frames_of)
    for i in range(6):
        a, b = together[i], solo[i]
        assert a["nr"] == b["nr"] == nrs[i] and not _nr_warnings(a["log"]), (i, a["log"])
        assert any("X264GPU_BATCH: stream" in t for _, t in a["log"]), "the session ran in a batch group"
        assert a["stream"] == b["stream"] and len(a["stream"]) > 0, f"session {i} (nr {nrs[i]}) codes other bytes in its group than alone"
        assert np.array_equal(a["offs"][-1], b["offs"][-1]) and bool(a["offs"][-1].any()) == (nrs[i] > 0), i
    assert together[0]["stream"] != together[2]["stream"]

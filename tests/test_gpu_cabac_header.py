"""GPU: the macroblock layer's own syntax in the CABAC size pricing (csrc/cabac_rd.hip.h cab_mb: mb_type, sub_mb_type, ref_idx, mvd, intra modes, cbp,
mb_qp_delta, transform-size flag and coded_block_flags collected as one bit string per context and walked through the chain table once a call).  Whole
pictures against the CPU checker — records, levels, reconstruction and the CABAC context variables after every picture (the comparisons of
test_gpu_pipeline and test_gpu_bframes.run) — on content chosen so that every kind of string occurs: each case first asserts, on the CHECKER's records
alone, that its content reaches the path it is there for."""
import ctypes as C
import functools

import numpy as np
import pytest

import bgop
import oracle_lib as O
from pan_content import pan_frames
from synth import synth_frames
from test_gpu_bframes import MEDIUM, run
from test_gpu_pipeline import CABAC_CTX_I, CABAC_CTX_P, compare

pytestmark = pytest.mark.gpu

IP = dict(cabac=1, rd=1, subme=7, partitions=7, dct8x8=1, refs=3, mixed_refs=1, chroma_me=1, psy=1, psy_rd_q8=256, chroma_qp_offset=-2, trellis=63)
KBX = [0, 1, 0, 1, 2, 3, 2, 3, 0, 1, 0, 1, 2, 3, 2, 3]
KBY = [0, 0, 1, 1, 0, 0, 1, 1, 2, 2, 3, 3, 2, 2, 3, 3]
KIDX = [[0, 1, 4, 5], [2, 3, 6, 7], [8, 9, 12, 13], [10, 11, 14, 15]]          # [by][bx]


# ---- the checker's side (CPU only; once per content and configuration) ----
class _Ctx(C.Structure):
    _fields_ = [("mbs", C.c_void_p), ("levels", C.c_void_p), ("mbw", C.c_int), ("mbh", C.c_int), ("first_row", C.c_int), ("pslice", C.c_int), ("num_ref", C.c_int),
                ("t8mode", C.c_int), ("amvd", C.c_void_p), ("state", C.c_void_p), ("last_dqp", C.c_int), ("last_qp", C.c_int), ("bslice", C.c_int),
                ("num_ref1", C.c_int), ("amvd1", C.c_void_p)]


def checker_amvd(mbs, lv, mbw, mbh, bslice, qp):
    """|mvd| (capped at 66 as x264 keeps it) of every 8x8 block, per list, [macroblock][list][block][x, y]: the checker's entropy coder run over its records in
    bitstream order (oracle/cabac_rd.cpp x264o_cabac_mb leaves them behind)"""
    O.L.x264o_cabac_mb.argtypes = [C.POINTER(_Ctx), C.c_int, C.c_int, C.c_int]
    O.L.x264o_cabac_mb.restype = C.c_long
    O.L.x264o_cabac_init_states.argtypes = [C.c_void_p, C.c_int, C.c_int]
    O.L.x264o_cabac_init_states.restype = None
    n = mbw * mbh
    st = np.zeros(460, np.uint8)
    O.L.x264o_cabac_init_states(st.ctypes.data, 1, qp)
    mbs, lv = np.ascontiguousarray(mbs), np.ascontiguousarray(lv)
    a0, a1 = np.zeros((n, 4, 2), np.uint8), np.zeros((n, 4, 2), np.uint8)
    c = _Ctx(mbs.ctypes.data, lv.ctypes.data, mbw, mbh, 0, 1, 3, 1, a0.ctypes.data, st.ctypes.data, 0, qp, bslice, 3, a1.ctypes.data)
    for i in range(n):
        O.L.x264o_cabac_mb(C.byref(c), i % mbw, i // mbw, 0)
    return np.stack([a0, a1], axis=1)


def mvd_stats(mbs, amvd):
    """how many vector differences reach the escape suffix (|mvd| >= 9), the most bins one macroblock puts on one of the two tail contexts (46: x, 53: y;
    a difference of 4 and up sends min(|mvd|, 9) - 4 ones there, and the closing zero below 9)"""
    tail = lambda a: np.where(a >= 4, np.minimum(a, 9) - 4 + (a < 9), 0)
    esc, most = 0, 0
    for i, m in enumerate(mbs):
        ty, part = int(m["type"]), int(m["partition"])
        if ty not in (O.MB_P_L0, O.MB_P_8x8, O.MB_B_INTER, O.MB_B_8x8):
            continue
        blocks = [0] if part == 0 else [0, 2] if part == 1 else [0, 1] if part == 2 else [0, 1, 2, 3]
        a = amvd[i][:, blocks, :].astype(np.int64)          # (a list or a direct block that sends nothing left zeros)
        esc += int((a >= 9).sum())
        most = max(most, int(tail(a[:, :, 0]).sum()), int(tail(a[:, :, 1]).sum()))
    return esc, most


def intra_pred_flags(mbs, mbw, i):
    """the sixteen prev_intra4x4_pred_mode flags of Intra_4x4 macroblock i (the checker's neighbour rule: oracle/cabac_rd.cpp pred_intra_mode)"""
    m, flags = mbs[i], []
    nb_mode = lambda n, blk: int(n["i4_mode"][blk]) if int(n["type"]) in (0, 1) else 2
    for b in range(16):
        bx, by = KBX[b], KBY[b]
        if bx > 0: ma = int(m["i4_mode"][KIDX[by][bx - 1]])
        elif i % mbw: ma = nb_mode(mbs[i - 1], KIDX[by][3])
        else: ma = None
        if by > 0: mb = int(m["i4_mode"][KIDX[by - 1][bx]])
        elif i >= mbw: mb = nb_mode(mbs[i - mbw], KIDX[3][bx])
        else: mb = None
        pred = 2 if ma is None or mb is None else min(ma, mb)
        flags.append(int(m["i4_mode"][b]) == pred)
    return flags


class _Keep:
    """an encoder that keeps what it returns"""
    def __init__(self, enc):
        self.enc, self.out = enc, []

    def encode_pic(self, f, pic):
        mbs, lv = self.enc.encode_pic(f, pic)
        self.out.append((mbs, lv))
        return mbs, lv

    def recon(self):
        return self.enc.recon()

    def direct_scores(self):
        return self.enc.direct_scores()


@functools.lru_cache(maxsize=None)
def _ip_records(content, w, h, n, seed, over):
    frames = content(w, h, n, seed)
    og = O.OracleEncoder(O.default_config(w, h, **dict(IP, **dict(over))))
    out = [og.encode(f, 2 if i == 0 else 0) for i, f in enumerate(frames)]
    og.close()
    return out


@functools.lru_cache(maxsize=None)
def _b_records(content, w, h, types, seed, over):
    """[(picture type, records, levels)] in coding order"""
    from x264vfw_amd import host_api as HL
    kw = dict(MEDIUM, **dict(over))
    cfg = O.default_config(w, h, **kw)
    keep = _Keep(O.OracleEncoder(cfg))
    order = bgop.encode_gop(HL, keep, content(w, h, len(types), seed), types, cfg, 20, 23, 25, kw["refs"], 3, 1)[2]
    return [(pt, mbs, lv) for (disp, pt), (mbs, lv) in zip(order, keep.out)]


def ip_run(gpu, w, h, frames, **over):
    """I then P pictures: device == checker, picture by picture"""
    from gpu_enc import GpuEncoder
    kw = dict(IP, **over)
    cfg = O.default_config(w, h, **kw)
    og, gg = O.OracleEncoder(cfg), GpuEncoder(cfg)
    ns = kw.get("slices", 1)
    for i, f in enumerate(frames):
        st = 2 if i == 0 else 0
        o_mb, o_lv = og.encode(f, st)
        g_mb, g_lv = gg.encode([f], st)
        compare(f"{w}x{h} {over} frame {i}", (w + 15) // 16, g_mb[0], o_mb, g_lv[0], o_lv, gg.recon(0), og.recon())
        used = CABAC_CTX_I if st == 2 else CABAC_CTX_P
        np.testing.assert_array_equal(gg.cabac_states(0, ns - 1)[used], og.cabac_states()[used], err_msg=f"context variables after picture {i}")
    og.close(); gg.close()


# ---- content ----
def synth(w, h, n, seed):
    return synth_frames(w, h, n, seed=seed)


def mixed_intra(w, h, n, seed):
    """flat, smooth and busy macroblocks side by side, a kind per macroblock drawn at random (flat grey | a ramp with a little noise | fine texture | 4x4
    patches of their own brightness | 4x4 blocks striped vertically and horizontally in turn), so that Intra_16x16, Intra_8x8 and Intra_4x4 all win
    somewhere, with every mode predicted in some macroblocks and none in others"""
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        yy, xx = np.mgrid[0:h, 0:w]
        kind = np.kron(rng.integers(0, 5, ((h + 15) // 16, (w + 15) // 16)), np.ones((16, 16), np.int64))[:h, :w]
        tex = rng.integers(16, 236, (h, w))
        ramp = 60 + (xx % 16) * 6 + (yy % 16) * 3 + rng.integers(-2, 3, (h, w))
        patch = np.kron(rng.integers(40, 200, ((h + 3) // 4, (w + 3) // 4)), np.ones((4, 4), np.int64))[:h, :w] + rng.integers(-2, 3, (h, w))
        turn = ((xx // 4) + (yy // 4)) & 1
        stripe = np.where(turn == 1, 60 + 120 * (xx & 1), 60 + 120 * (yy & 1)) + rng.integers(-2, 3, (h, w))
        # the four macroblocks at the origin: columns of random brightness, stepped every four rows — vertical prediction block by block, so the fourth
        # of them has every mode predicted from its neighbours
        kind[:32, :32] = 5
        cols = np.broadcast_to(rng.integers(40, 180, w), (h, w)) + 9 * ((yy // 4) % 6)
        y = np.where(kind == 0, 128, np.where(kind == 1, ramp, np.where(kind == 2, tex, np.where(kind == 3, patch, np.where(kind == 4, stripe, cols)))))
        u = np.full((h // 2, w // 2), 120) + rng.integers(-3, 4, (h // 2, w // 2))
        v = np.full((h // 2, w // 2), 136) + rng.integers(-3, 4, (h // 2, w // 2))
        out.append(np.concatenate([np.clip(p, 16, 235).astype(np.uint8).ravel() for p in (y, u, v)]))
    return out


def fast_pan(w, h, n, seed):
    return pan_frames(w, h, n, seed, 9, 6, 6)


def noisy_pan(w, h, n, seed):
    return pan_frames(w, h, n, seed, 2, -1, 14)


# ---- (a) + (g) I pictures: the three intra types, all modes predicted / none predicted, 8x8 transform on and off ----
def _intra_stats(content, w, h, seed, **over):
    mbs = _ip_records(content, w, h, 1, seed, tuple(sorted(over.items())))[0][0]
    ty = mbs["type"]
    fl = [sum(intra_pred_flags(mbs, (w + 15) // 16, i)) for i in np.nonzero(ty == 0)[0]]
    return dict(i4=int((ty == 0).sum()), i8=int((ty == 1).sum()), i16=int((ty == 2).sum()), all_pred=fl.count(16), none_pred=fl.count(0),
                cmodes=len(set(mbs["chroma_mode"].tolist())))


@pytest.mark.parametrize("w,h", [(64, 48), (96, 64)])
def test_i_picture_three_intra_types_modes_predicted_and_not(gpu, w, h):
    st = _intra_stats(mixed_intra, w, h, 67)
    print(st)
    assert st["i4"] >= 2 and st["i8"] >= 1 and st["i16"] >= 1 and st["all_pred"] >= 1 and st["none_pred"] >= 1, st
    ip_run(gpu, w, h, mixed_intra(w, h, 1, 67))


SIZES = [(64, 48), (96, 64)]


@pytest.mark.parametrize("w,h", SIZES)
def test_i_picture_without_8x8dct(gpu, w, h):
    st = _intra_stats(mixed_intra, w, h, 67, dct8x8=0, partitions=3)
    print(st)
    assert st["i4"] >= 2 and st["i8"] == 0 and st["i16"] >= 1, st
    ip_run(gpu, w, h, mixed_intra(w, h, 1, 67), dct8x8=0, partitions=3)


# ---- (b) P pictures: three references, the four partition shapes, P_8x8 ----
def _p_stats(content, w, h, n, seed, **over):
    s = dict(shapes=set(), refs=set(), p8x8=0, esc=0, most=0, dqp=set(), t8=set())
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    kw = dict(IP, **over)
    for k, (mbs, lv) in enumerate(_ip_records(content, w, h, n, seed, tuple(sorted(over.items())))):
        if k == 0:
            continue
        inter = (mbs["type"] == O.MB_P_L0) | (mbs["type"] == O.MB_P_8x8)
        s["shapes"] |= set(mbs["partition"][inter].tolist())
        s["refs"] |= set(mbs["ref"][inter].ravel().tolist()) - {-1}
        s["p8x8"] += int((mbs["type"] == O.MB_P_8x8).sum())
        s["t8"] |= set(mbs["transform8x8"][inter & (mbs["cbp_luma"] != 0)].tolist())
        if kw.get("slices", 1) == 1:
            esc, most = mvd_stats(mbs, checker_amvd(mbs, lv, mbw, mbh, 0, kw.get("qp_p", 23)))
            s["esc"] += esc; s["most"] = max(s["most"], most)
        coded = (mbs["cbp_luma"] != 0) | (mbs["cbp_chroma"] != 0)
        q = mbs["qp"][coded].astype(int)
        s["dqp"] |= set(np.sign(np.diff(q)).tolist())
    return s


@pytest.mark.parametrize("w,h", SIZES)
def test_p_pictures_three_references_every_shape(gpu, w, h):
    st = _p_stats(synth, w, h, 5, 1)
    print(st)
    assert st["shapes"] == {0, 1, 2, 3} and st["p8x8"] >= 2 and st["refs"] >= {0, 1, 2} and st["t8"] == {0, 1}, st          # (the transform-size flag both ways)
    ip_run(gpu, w, h, synth(w, h, 5, 1))


@pytest.mark.parametrize("w,h", SIZES)
def test_p_pictures_without_8x8dct(gpu, w, h):
    st = _p_stats(synth, w, h, 3, 1, dct8x8=0)
    print(st)
    assert st["p8x8"] >= 1 and st["t8"] <= {0}, st
    ip_run(gpu, w, h, synth(w, h, 3, 1), dct8x8=0)


# ---- (e) aq-mode 1: mb_qp_delta in both signs ----
@pytest.mark.parametrize("w,h", SIZES)
def test_p_pictures_aq_mode_1_qp_delta_both_signs(gpu, w, h):
    st = _p_stats(mixed_intra, w, h, 3, 5, aq_mode=1)
    print(st)
    assert {-1, 1} <= st["dqp"], st
    ip_run(gpu, w, h, mixed_intra(w, h, 3, 5), aq_mode=1)


# ---- (f) RD refinement in P (subme 8): parts priced on their own (in.pm 1: P parts; 2 / 3: Intra_4x4 / Intra_8x8 blocks; 4: intra chroma) ----
@pytest.mark.parametrize("w,h", SIZES)
def test_p_pictures_rd_refinement(gpu, w, h):
    st = _p_stats(synth, w, h, 3, 1, subme=8, rd=63)
    print(st)
    assert len(st["shapes"]) >= 3 and st["p8x8"] >= 1, st
    ip_run(gpu, w, h, synth(w, h, 3, 1), subme=8, rd=63)
    st = _intra_stats(mixed_intra, w, h, 67, subme=8, rd=63)
    assert st["i4"] >= 1 and st["i8"] >= 1 and st["i16"] >= 1, st
    ip_run(gpu, w, h, mixed_intra(w, h, 2, 67), subme=8, rd=63)


# ---- (h) three slices ----
def test_p_pictures_three_slices(gpu):
    st = _p_stats(synth, 96, 192, 3, 1, slices=3)
    print(st)
    assert st["p8x8"] >= 2 and len(st["shapes"]) >= 3, st
    ip_run(gpu, 96, 192, synth(96, 192, 3, 1), slices=3)


# ---- (c) + (d) B pictures ----
def _b_stats(content, w, h, types, seed, **over):
    """b8x8: B_8x8 macroblocks; sub: their sub-block kinds; mixed: 16x8 / 8x16 macroblocks whose halves use different lists; bi_parts: bi-predicted parts of
    B_8x8 and 16x8 / 8x16 macroblocks (RD refinement prices such a part with both lists' differences); esc / most: mvd_stats over P and B pictures"""
    s = dict(b8x8=0, sub=set(), mixed=0, bi_parts=0, esc=0, most=0)
    mbw, mbh = (w + 15) // 16, (h + 15) // 16
    kw = dict(MEDIUM, **over)
    for pt, mbs, lv in _b_records(content, w, h, types, seed, tuple(sorted(over.items()))):
        if pt < 2:
            continue
        if kw.get("slices", 1) == 1:
            esc, most = mvd_stats(mbs, checker_amvd(mbs, lv, mbw, mbh, pt >= 3, bgop.pic_qp(pt, 20, 23, 25)))
            s["esc"] += esc; s["most"] = max(s["most"], most)
        if pt < 3:
            continue
        r0, r1 = mbs["ref"], O.mb_ref1(mbs)
        for i in np.nonzero(mbs["type"] == O.MB_B_8x8)[0]:
            s["b8x8"] += 1
            for k in range(4):
                kind = "direct" if (int(mbs["i16_mode"][i]) >> k) & 1 else "bi" if r0[i][k] >= 0 and r1[i][k] >= 0 else "l0" if r0[i][k] >= 0 else "l1"
                s["sub"].add(kind)
                s["bi_parts"] += kind == "bi"
        for i in np.nonzero((mbs["type"] == O.MB_B_INTER) & ((mbs["partition"] == 1) | (mbs["partition"] == 2)))[0]:
            k2 = 2 if mbs["partition"][i] == 1 else 1
            use = lambda k: (bool(r0[i][k] >= 0), bool(r1[i][k] >= 0))
            s["mixed"] += use(0) != use(k2)
            s["bi_parts"] += (use(0) == (True, True)) + (use(k2) == (True, True))
    return s


@pytest.mark.parametrize("w,h", SIZES)
def test_b_pictures_b8x8_sub_types_and_mixed_lists(gpu, w, h):
    st = _b_stats(synth, w, h, "IBBBPBBBP", 1)
    print(st)
    assert st["b8x8"] >= 2 and st["sub"] == {"direct", "l0", "l1", "bi"} and st["mixed"] >= 1, st
    run(gpu, w, h, "IBBBPBBBP", 1, frames=synth(w, h, 9, 1))


@pytest.mark.parametrize("w,h", SIZES)
def test_fast_pan_escape_suffix_and_long_mvd_tails(gpu, w, h):
    st = _b_stats(fast_pan, w, h, "IBBBPBBBP", 1)
    print(st)
    assert st["esc"] >= 10 and st["most"] > 32, st          # (more than 32 bins on context 46 or 53 in one macroblock: a B_8x8 with long differences in both lists)
    run(gpu, w, h, "IBBBPBBBP", 1, frames=fast_pan(w, h, 9, 1))


@pytest.mark.parametrize("w,h", SIZES)
def test_b_pictures_rd_refinement(gpu, w, h):
    st = _b_stats(synth, w, h, "IBBBP", 1, subme=9, rd=63)
    print(st)
    assert st["b8x8"] >= 1 and st["mixed"] >= 1 and st["bi_parts"] >= 2, st          # (parts with one list and with both: in.pm 1 with pm_lists 1, 2 and 3)
    run(gpu, w, h, "IBBBP", 1, frames=synth(w, h, 5, 1), subme=9, rd=63)


@pytest.mark.parametrize("w,h", SIZES)
def test_b_pictures_without_8x8dct(gpu, w, h):
    st = _b_stats(synth, w, h, "IBBBP", 1, dct8x8=0)
    print(st)
    assert st["b8x8"] >= 1, st
    run(gpu, w, h, "IBBBP", 1, frames=synth(w, h, 5, 1), dct8x8=0)


def test_b_pictures_three_slices(gpu):
    st = _b_stats(synth, 96, 192, "IBBBP", 1, slices=3)
    print(st)
    assert st["b8x8"] >= 2, st
    run(gpu, 96, 192, "IBBBP", 1, frames=synth(96, 192, 5, 1), slices=3)

"""-m gpu: psy-trellis (--psy-rd a:b; cfg.psy_trellis_q8) on the device against the pure-Python twin of the search (tests/trellis_psy_ref.py, itself pinned to
oracle/trellis.cpp at strength 0 by tests/test_trellis_psy_cpu.py): the primitive x264gpu_trellis_blocks_psy, the source transform the macroblock loop hands
every luma trellis site, and whole sessions through x264_encoder_encode."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import trellis_psy_ref as T

pytestmark = pytest.mark.gpu


# ---- (3) the primitive ----
def _device(lib, cat, qp, intra, coefs, states, psy, fenc, force_general=0, entry="psy"):
    import torch
    nblk = len(coefs)
    d_c, d_s = torch.from_numpy(coefs.copy()).cuda(), torch.from_numpy(states).cuda()
    d_f = torch.from_numpy(fenc.copy()).cuda() if fenc is not None else None
    d_l, d_z = torch.zeros_like(d_c), torch.zeros(nblk, dtype=torch.uint8, device="cuda")
    d_p = torch.full(((nblk + 7) // 8,), 0xff, dtype=torch.uint8, device="cuda")
    if entry == "psy":
        lib.check(lib.x264gpu_trellis_blocks_psy(d_c.data_ptr(), d_f.data_ptr() if d_f is not None else None, nblk, cat, qp, intra, psy, d_s.data_ptr(), d_l.data_ptr(),
                                                 d_z.data_ptr(), force_general, d_p.data_ptr(), None), "trellis_blocks_psy")
    else:
        lib.check(lib.x264gpu_trellis_blocks_ex(d_c.data_ptr(), nblk, cat, qp, intra, d_s.data_ptr(), d_l.data_ptr(), d_z.data_ptr(), force_general, d_p.data_ptr(), None),
                  "trellis_blocks_ex")
    torch.cuda.synchronize()
    return d_l.cpu().numpy(), d_z.cpu().numpy(), d_p.cpu().numpy()


def _fenc(cat, shape, rng):
    """what a transform of 8-bit samples can hold (4x4: |.| <= 36 * 255 / 2, 8x8 a few times that), independent of the coefficients"""
    return rng.integers(-12000, 12001, shape).astype(np.int16) if cat == 5 else rng.integers(-4500, 4501, shape).astype(np.int16)


def _inputs(cat, qp, intra, kind):
    rng = np.random.default_rng(4000 + 100 * cat + 2 * qp + intra + (7 if kind == "sparse" else 0))
    nblk = 6 if cat == 5 else 13                       # 16-coefficient categories: one full pass of eight blocks and a partial one
    coefs = T.random_blocks(cat, qp, kind, 16, rng)[:nblk]
    return coefs, T.random_states(rng), _fenc(cat, coefs.shape, rng)


_TWIN = {}


def _twin(cat, qp, intra, kind, psy):
    key = (cat, qp, intra, kind, psy)
    if key not in _TWIN:
        coefs, states, fenc = _inputs(cat, qp, intra, kind)
        _TWIN[key] = T.quant_trellis_blocks(coefs, cat, qp, intra, states, psy, fenc)
    return _TWIN[key]


@pytest.mark.parametrize("psy", [10, 45, 640])
@pytest.mark.parametrize("qp,intra", [(20, 1), (20, 0), (37, 1), (37, 0)])
@pytest.mark.parametrize("cat", [1, 2, 5])
def test_primitive_equals_twin(gpu, cat, qp, intra, psy):
    for kind in ("dense", "sparse"):
        coefs, states, fenc = _inputs(cat, qp, intra, kind)
        want, want_nz = _twin(cat, qp, intra, kind, psy)
        for force in (0, 1):
            got, got_nz, paths = _device(gpu, cat, qp, intra, coefs, states, psy, fenc, force)
            bad = np.nonzero((got != want).any(axis=1))[0]
            assert len(bad) == 0, (f"{kind} force_general {force}: {len(bad)} of {len(want)} blocks differ; first {bad[0]}: coefs {coefs[bad[0]].tolist()} fenc "
                                   f"{fenc[bad[0]].tolist()} device {got[bad[0]].tolist()} twin {want[bad[0]].tolist()}")
            np.testing.assert_array_equal(got_nz, want_nz)
            if force: assert (paths == 0).all()
            elif kind == "sparse": assert (paths == 1).all(), "every guess is 0 or 1: the levels-of-one loop"
            else: assert not paths.any()
        assert np.count_nonzero(want) > 0


def test_the_psy_term_is_felt(gpu):
    """the cases above are not vacuous: at the largest strength the twin's levels differ from the plain search's in every category and kind of input"""
    for cat in (1, 2, 5):
        for kind in ("dense", "sparse"):
            coefs, states, fenc = _inputs(cat, 20, 1, kind)
            plain, _ = T.quant_trellis_blocks(coefs, cat, 20, 1, states)
            assert not np.array_equal(plain, _twin(cat, 20, 1, kind, 640)[0]), (cat, kind)


@pytest.mark.parametrize("cat", [0, 1, 2, 3, 4, 5])
def test_strength_0_and_untouched_categories_equal_the_plain_entry(gpu, cat):
    for kind in ("dense", "sparse"):
        rng = np.random.default_rng(600 + cat)
        coefs, states = T.random_blocks(cat, 26, kind, 16, rng)[:6 if cat == 5 else 13], T.random_states(rng)
        fenc = _fenc(cat, coefs.shape, rng)
        for force in (0, 1):
            ex = _device(gpu, cat, 26, 0, coefs, states, 0, None, force, entry="ex")
            z = _device(gpu, cat, 26, 0, coefs, states, 0, fenc, force)
            assert all(a.tobytes() == b.tobytes() for a, b in zip(ex, z)), "strength 0"
            if cat in (0, 3, 4):
                nzp = _device(gpu, cat, 26, 0, coefs, states, 640, fenc, force)
                assert all(a.tobytes() == b.tobytes() for a, b in zip(ex, nzp)), "a category without the psy term"


# ---- (4) the macroblock loop hands each site the right source blocks ----
MBW, MBH, QP = 1, 8, 20          # the narrowest picture the encoder takes, one slice per macroblock row: every macroblock is the first of a slice
BLK_XY = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0), (2, 1), (3, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 2), (3, 2), (2, 3), (3, 3)]          # 4x4 block order -> (bx, by)
CF4 = np.array([[1, 1, 1, 1], [2, 1, -1, -2], [1, -1, -1, 1], [1, -2, 2, -1]], np.int64)


def first_mb_frames():
    """two streams of 16 x 128 luma: per macroblock a level near 128, a gentle ramp, a faint 2 x 2 checker and mild noise whose strength varies from
    macroblock to macroblock.  No Intra_4x4 / Intra_8x8 mode predicts the checker better than Intra_16x16's flat 128, so most macroblocks are cheapest as
    Intra_16x16 with AC levels to search; the noisier ones go to Intra_4x4 / Intra_8x8 (confirmed on the CPU checker at strength 0:
    tests/test_trellis_psy_cpu.py::test_first_macroblock_source_gives_mostly_intra_16x16)"""
    frames = []
    yy, xx = np.mgrid[0:16, 0:16]
    chk = 2 * (((xx >> 1) + (yy >> 1)) & 1) - 1
    for s in range(2):
        rng = np.random.default_rng(77 + s)
        w, h = 16 * MBW, 16 * MBH
        y = np.zeros((h, w))
        for m in range(MBH):
            sigma = [1.5, 3.0, 1.5, 2.5, 5.0, 1.5, 3.0, 6.0][(m + 3 * s) % 8]
            y[16 * m:16 * m + 16] = 128 + rng.integers(-2, 3) + rng.integers(3, 6) * chk + rng.uniform(-0.25, 0.25) * (xx - 7.5) + rng.normal(0, sigma, (16, 16))
        f = np.full(w * h * 3 // 2, 128, np.uint8)
        f[:w * h] = np.clip(np.rint(y), 0, 255).astype(np.uint8).ravel()
        frames.append(f)
    return frames


def first_mb_config(psy):
    return O.default_config(16 * MBW, 16 * MBH, streams=2, qp_i=QP, partitions=7, dct8x8=1, cabac=1, rd=1, subme=7, psy=1, psy_rd_q8=256, chroma_qp_offset=-2, trellis=63,
                            me_method=1, slices=MBH, slices_plain=1, psy_trellis_q8=psy)


def dct4(x):
    return CF4 @ x.astype(np.int64) @ CF4.T


def dct8(x, pred):
    out = np.zeros(64, np.int16)
    e, p = np.ascontiguousarray(x, np.uint8), np.full((8, 8), pred, np.uint8)
    O.L.x264o_sub8x8_dct8.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int]
    O.L.x264o_sub8x8_dct8.restype = None
    O.L.x264o_sub8x8_dct8(out.ctypes.data, e.ctypes.data, 8, p.ctypes.data, 8)
    return out.astype(np.int64)


def expected_first_mb_levels(src16, mb_type, t8x8, psy):
    """-> [(offset into the macroblock's levels, expected levels)] of the blocks whose prediction is known from outside (flat 128): all sixteen AC blocks of an
    Intra_16x16 macroblock, block 0 of an Intra_4x4 / Intra_8x8 one.  The context variables are the slice's initial ones"""
    st = np.zeros(460, np.uint8)
    O.L.x264o_cabac_init_states.argtypes = [C.c_void_p, C.c_int, C.c_int]
    O.L.x264o_cabac_init_states.restype = None
    O.L.x264o_cabac_init_states(st.ctypes.data, 0, QP)
    out = []
    zz4 = np.array(T.ZZ4)
    if mb_type == 2:
        for b, (bx, by) in enumerate(BLK_XY):
            blk = src16[4 * by:4 * by + 4, 4 * bx:4 * bx + 4].astype(np.int64)
            res, fen = dct4(blk - 128).ravel()[zz4], dct4(blk).ravel()[zz4]
            out.append((b * 16 + 1, T.quant_trellis(res.tolist(), 1, QP, 1, st, psy, fen.tolist())[1:]))          # (entry 0 of an AC block is not a level)
    elif mb_type == 0:
        blk = src16[:4, :4].astype(np.int64)
        out.append((0, T.quant_trellis(dct4(blk - 128).ravel()[zz4].tolist(), 2, QP, 1, st, psy, dct4(blk).ravel()[zz4].tolist())))
    else:
        zz8 = np.array(T.ZZ8)
        lv = T.quant_trellis(dct8(src16[:8, :8], 128)[zz8].tolist(), 5, QP, 1, st, psy, dct8(src16[:8, :8], 0)[zz8].tolist())
        inter = np.zeros(64, np.int64)          # 8x8 block 0 in the interleaved form: level z of the zigzag at block z & 3, entry z >> 2
        for z in range(64):
            inter[(z & 3) * 16 + (z >> 2)] = lv[z]
        out.append((0, inter.tolist()))
    return out


def _check_first_mbs(mbs, lvs, frames, psy):
    n16 = nchecked = 0
    for s in range(2):
        y = frames[s][:16 * MBW * 16 * MBH].reshape(16 * MBH, 16 * MBW)
        for m in range(MBH):
            t = int(mbs[s][m]["type"])
            assert t in (0, 1, 2)
            assert (t == 1) == bool(mbs[s][m]["transform8x8"]) or mbs[s][m]["cbp_luma"] == 0
            n16 += t == 2
            for off, want in expected_first_mb_levels(y[16 * m:16 * m + 16, :16], t, t == 1, psy):
                got = lvs[s][m][off:off + len(want)].tolist()
                assert got == want, f"stream {s} macroblock {m} type {t} levels at {off}: device {got} twin {want}"
                nchecked += 1
    return n16, nchecked


def test_first_macroblocks_of_slices_use_their_source_transform(gpu):
    from gpu_enc import GpuEncoder
    frames = first_mb_frames()
    got = {}
    for psy in (45, 0):
        gg = GpuEncoder(first_mb_config(psy))
        mbs, lvs = gg.encode(frames, O.SLICE_I)
        got[psy] = (mbs.copy(), lvs.copy())
        gg.close()
        n16, nchecked = _check_first_mbs(mbs, lvs, frames, psy)
        assert 2 * n16 >= 2 * MBH and n16 < 2 * MBH, f"{n16} of {2 * MBH} first macroblocks are Intra_16x16: the source must give mostly these, and some of the others"
        assert nchecked >= 16 * n16
    # the analysis runs before the final encode: the modes do not depend on the strength; the levels do
    assert np.array_equal(got[45][0]["type"], got[0][0]["type"])
    assert not np.array_equal(got[45][1][:, :, :256], got[0][1][:, :, :256]), "psy-trellis 45 changed no luma level"


# ---- (5) whole sessions ----
def _session(tune, opts, w=64, h=48, n=7):
    import host_lib as HL
    from quality_sessions import make_logger
    from synth import synth_frames
    H = HL.H
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", tune) == 0
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
            assert H.x264host_get_recon(h_, rec.ctypes.data) == 0
            recons.append(rec); types.append(int(out.i_type))
    for i, f in enumerate(synth_frames(w, h, n, seed=11)):
        C.memmove(pic.img.plane[0], f.ctypes.data, f.size)
        pic.i_pts = i
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), C.byref(pic), C.byref(out)))
    while H.x264_encoder_delayed_frames(h_):
        take(H.x264_encoder_encode(h_, C.byref(nal), C.byref(nn), None, C.byref(out)))
    H.x264_encoder_close(h_)
    H.x264_picture_clean(C.byref(pic))
    return dict(stream=stream, recons=recons, types=types, log=log, psy_trellis=eff.analyse.f_psy_trellis, cqo=eff.analyse.i_chroma_qp_offset, me=eff.analyse.i_me_method,
                trellis=eff.analyse.i_trellis)


def pps_chroma_qp_index_offset(stream):
    """7.3.2.2 up to chroma_qp_index_offset (one slice group)"""
    from hrd_ref import Bits, split_annexb
    rbsp = [r for _, t, r, _ in split_annexb(stream) if t == 8][0]
    b = Bits(rbsp)
    b.ue(); b.ue(); b.u(1); b.u(1)
    assert b.ue() == 0
    b.ue(); b.ue(); b.u(1); b.u(2); b.se(); b.se()
    return b.se()


@pytest.mark.parametrize("tune,opts,strength,drop", [(b"film", {"qp": 24, "keyint": 30, "b-adapt": 0}, 0.15, 1),
                                                    (None, {"qp": 24, "keyint": 30, "b-adapt": 0, "me": "umh", "subme": 9, "trellis": 2, "psy-rd": "1.0:0.25"}, 0.25, 2)])
def test_sessions_with_psy_trellis(gpu, tune, opts, strength, drop):
    n, w, h = 7, 64, 48
    a = _session(tune, opts)
    assert abs(a["psy_trellis"] - strength) < 1e-6 and a["trellis"] == opts.get("trellis", 1) and a["me"] == (2 if "me" in opts else 1)
    assert not [m for lvl, m in a["log"] if "psy-trellis" in m], a["log"]
    assert len(a["recons"]) == n and 5 in a["types"], f"picture types {a['types']}: the session must hold B pictures"
    dec = O.h264_decode(a["stream"], n, w, h)
    assert len(dec) == n
    for i in range(n):
        np.testing.assert_array_equal(dec[i], a["recons"][i], err_msg=f"decoded picture {i} != encoder reconstruction")
    b = _session(tune, dict(opts, **{"psy-rd": "1.0:0"}))
    assert b["psy_trellis"] == 0 and b["stream"] != a["stream"]
    assert a["cqo"] == b["cqo"] - drop
    assert pps_chroma_qp_index_offset(a["stream"]) == a["cqo"] and pps_chroma_qp_index_offset(b["stream"]) == b["cqo"]

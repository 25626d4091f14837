"""Pure-Python twin of x264's noise reduction (--nr; [x264-upstream] common/quant.c denoise_dct, encoder/encoder.c x264_noise_reduction_update) as the
device runs it (include/x264gpu.h x264gpu_encoder_set_nr / x264gpu_nr_update / x264gpu_denoise_blocks), in numpy and Python integers.

Categories: 0 = luma 4x4 (16 entries), 1 = luma 8x8 (64), 2 = chroma 4x4 (16); the index is the raster position in the block's transform array.
Two stated choices differ from x264: an offset is stored as min(value, 32767) (x264 lets a uint16 wrap), and the statistics take the final encode of the inter
macroblocks that are not skips (x264 adds every denoise call, RD candidates and probes included).  Test infrastructure."""
import ctypes as C

import numpy as np

from trellis_psy_ref import CLS8, W2_4, W2_8

NCOEF = (16, 64, 16)
THRESH = (1 << 18, 1 << 16, 1 << 18)
OFF_MAX = 32767


def weight2(cat, i):
    """coef_weight2 of raster index i (the trellis search's distortion weights, FIX8)"""
    if cat == 1:
        return W2_8[CLS8[(i >> 3) & 3][i & 3]]
    return W2_4[((i >> 2) & 1) + (i & 1)]


def zero_state():
    return {"sum": [[0] * 64 for _ in range(3)], "count": [0, 0, 0]}


def zero_offsets():
    return np.zeros((3, 64), np.uint16)


def denoise(block, cat, offsets, sums=None):
    """block: the coefficients of one block in raster order; returns the denoised block (int16) and adds |coefficient| (as it was) into sums[cat]"""
    out = np.zeros(NCOEF[cat], np.int16)
    for i in range(NCOEF[cat]):
        d = int(block[i])
        a = abs(d)
        if sums is not None:
            sums["sum"][cat][i] += a
        a -= int(offsets[cat][i])
        out[i] = 0 if a < 0 else (-a if d < 0 else a)
    return out


def denoise_blocks(blocks, cat, offsets):
    """-> (denoised blocks, sums of this call alone: count[cat] = the number of blocks)"""
    sums = zero_state()
    out = np.stack([denoise(b, cat, offsets, sums) for b in blocks])
    sums["count"][cat] = len(blocks)
    return out, sums


def update(state, pic, strength):
    """state += pic (pic None: the state as it is), the halving rule, the new offsets.  Changes `state`; returns the offsets [3][64] uint16"""
    off = zero_offsets()
    for cat in range(3):
        if pic is not None:
            state["count"][cat] += int(pic["count"][cat])
            for i in range(NCOEF[cat]):
                state["sum"][cat][i] += int(pic["sum"][cat][i])
        if state["count"][cat] > THRESH[cat]:
            state["sum"][cat] = [v >> 1 for v in state["sum"][cat]]
            state["count"][cat] >>= 1
        for i in range(1, NCOEF[cat]):
            s = state["sum"][cat][i]
            off[cat][i] = min((strength * state["count"][cat] + s // 2) // (s * weight2(cat, i) // 256 + 1), OFF_MAX)
    return off


def sums_struct(s):
    """a sums dictionary as the bytes of x264gpu_nr_sums"""
    a = np.zeros(3 * 64, np.uint64)
    for cat in range(3):
        a[cat * 64:cat * 64 + 64] = np.array(s["sum"][cat], np.uint64)
    return a.tobytes() + np.array(list(s["count"]) + [0], np.uint32).tobytes()


def sums_from_bytes(buf):
    a = np.frombuffer(buf[:1536], np.uint64).reshape(3, 64)
    c = np.frombuffer(buf[1536:1552], np.uint32)
    return {"sum": [[int(v) for v in a[cat]] for cat in range(3)], "count": [int(c[0]), int(c[1]), int(c[2])]}


# ---- the statistics of a coded P picture, recomputed from its records ----
BLK_XY = [(0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0), (2, 1), (3, 1), (0, 2), (1, 2), (0, 3), (1, 3), (2, 2), (3, 2), (2, 3), (3, 3)]          # 4x4 block order -> (bx, by)


_DCT = {}


def _dct(O, name, n, src, pred):
    """x264o_sub4x4_dct / x264o_sub8x8_dct8 of the checker library through a binding of this module's own (a handle of its own: the signature set here is not
    the one other test modules see or change)"""
    if name not in _DCT:
        fn = getattr(C.CDLL(O.L._name), name)
        fn.argtypes, fn.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_void_p, C.c_int], None
        _DCT[name] = fn
    out = np.zeros(n * n, np.int16)
    e, p = np.ascontiguousarray(src, np.uint8), np.ascontiguousarray(pred, np.uint8)
    _DCT[name](out.ctypes.data, e.ctypes.data, n, p.ctypes.data, n)
    return out


def picture_sums(O, src, ref, mbs, w, h):
    """the statistics of a P picture with one reference and no weights, from its records alone: src = the source picture, ref = the reference's reconstruction
    (both tight I420, w and h multiples of 16), mbs = the picture's records.  Every inter macroblock that is not P_Skip: the prediction of its four 8x8 blocks at
    their vectors (x264o_frame_filter / x264o_mc_luma / x264o_mc_chroma), the residual transformed with the size the record names.  (A macroblock coded with the
    8x8 transform that left no luma level is recorded without transform_size_8x8_flag: it counts as 4x4 blocks, on the device too.)"""
    assert w % 16 == 0 and h % 16 == 0
    pad, cpad = 32, 16
    planes, stride = O.make_padded_planes(ref[:w * h].reshape(h, w), pad)
    O.frame_filter(planes, stride, w, h, pad)
    pp = O.plane_ptrs(planes, stride, pad)
    cw, ch = w // 2, h // 2
    u, v = ref[w * h:w * h + cw * ch].reshape(ch, cw), ref[w * h + cw * ch:].reshape(ch, cw)
    nv = np.zeros((ch + 2 * cpad, 2 * (cw + 2 * cpad)), np.uint8)
    nv[:, 0::2], nv[:, 1::2] = np.pad(u, cpad, mode="edge"), np.pad(v, cpad, mode="edge")
    org = cpad * nv.shape[1] + 2 * cpad
    sy = src[:w * h].reshape(h, w)
    su, sv = src[w * h:w * h + cw * ch].reshape(ch, cw), src[w * h + cw * ch:].reshape(ch, cw)
    sums = zero_state()
    mbw = w // 16
    for i, m in enumerate(mbs):
        if int(m["type"]) not in (O.MB_P_L0, O.MB_P_8x8):
            continue
        mbx, mby = i % mbw, i // mbw
        py, pu, pv = np.zeros((16, 16), np.uint8), np.zeros((8, 8), np.uint8), np.zeros((8, 8), np.uint8)
        for b in range(4):
            assert int(m["ref"][b]) == 0
            bx, by, mvx, mvy = 8 * (b & 1), 8 * (b >> 1), int(m["mv"][b][0]), int(m["mv"][b][1])
            blk = np.zeros((8, 8), np.uint8)
            O.L.x264o_mc_luma(O.ptr(blk), 8, pp, stride, 16 * mbx + bx, 16 * mby + by, mvx, mvy, 8, 8)
            py[by:by + 8, bx:bx + 8] = blk
            cu, cv = np.zeros((4, 4), np.uint8), np.zeros((4, 4), np.uint8)
            O.L.x264o_mc_chroma(O.ptr(cu), O.ptr(cv), 4, O.ptr(nv, org), nv.shape[1], 8 * mbx + bx // 2, 8 * mby + by // 2, mvx, mvy, 4, 4)
            pu[by // 2:by // 2 + 4, bx // 2:bx // 2 + 4], pv[by // 2:by // 2 + 4, bx // 2:bx // 2 + 4] = cu, cv
        mb_sums(O, sy[16 * mby:16 * mby + 16, 16 * mbx:16 * mbx + 16], su[8 * mby:8 * mby + 8, 8 * mbx:8 * mbx + 8], sv[8 * mby:8 * mby + 8, 8 * mbx:8 * mbx + 8],
                py, pu, pv, bool(m["transform8x8"]), sums)
    return sums


def mb_sums(O, src_y, src_u, src_v, pred_y, pred_u, pred_v, t8, sums):
    """adds one inter macroblock's final-encode statistics: 16x16 source / prediction luma, 8x8 chroma planes; t8: the 8x8 transform"""
    if t8:
        for b in range(4):
            x, y = 8 * (b & 1), 8 * (b >> 1)
            d = _dct(O, "x264o_sub8x8_dct8", 8, src_y[y:y + 8, x:x + 8], pred_y[y:y + 8, x:x + 8])
            for i in range(64):
                sums["sum"][1][i] += abs(int(d[i]))
        sums["count"][1] += 4
    else:
        for bx, by in BLK_XY:
            d = _dct(O, "x264o_sub4x4_dct", 4, src_y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4], pred_y[4 * by:4 * by + 4, 4 * bx:4 * bx + 4])
            for i in range(16):
                sums["sum"][0][i] += abs(int(d[i]))
        sums["count"][0] += 16
    for s, p in ((src_u, pred_u), (src_v, pred_v)):
        for b in range(4):
            x, y = 4 * (b & 1), 4 * (b >> 1)
            d = _dct(O, "x264o_sub4x4_dct", 4, s[y:y + 4, x:x + 4], p[y:y + 4, x:x + 4])
            for i in range(16):
                sums["sum"][2][i] += abs(int(d[i]))
    sums["count"][2] += 8

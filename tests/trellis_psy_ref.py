"""Serial restatement of the CABAC trellis quantiser as oracle/TRELLIS_NOTES.md states it ([x264-upstream] encoder/rdo.c quant_trellis_cabac), every
category, the DC-only shortcut and the escape suffix, with the psy-trellis term (--psy-rd a:b; oracle/trellis.cpp's x264o_quant_trellis_cabac_psy is a third statement of it): in luma blocks that
are not DC blocks (categories 1, 2, 5), at scan positions i > 0, a candidate level pays

    d * d * coef_weight2[zz] - coef_weight1[zz] * i_psy_trellis * abs(unquant_abs_level + SIGN(fenc_dct[zz] - coef, coef))

instead of d * d * coef_weight2[zz] (fenc_dct = the transform of the SOURCE block, coef = the signed residual coefficient).  It is pinned to
oracle/trellis.cpp block for block, at strength 0 and above (tests/test_trellis_psy_cpu.py); the device's x264gpu_trellis_blocks_psy and the macroblock loop are checked against it.
Test infrastructure: pure Python, blocks in SCAN order; the entropy table is csrc/cabac_entropy.inc, the 8x8 context increments host/cabac_tables.hpp."""
import os
import re

_HERE = os.path.dirname(os.path.abspath(__file__))
_PKG = os.path.join(_HERE, "..", "x264vfw_amd")
ENT = [int(x) for x in re.findall(r"\d+", "".join(l for l in open(os.path.join(_PKG, "csrc", "cabac_entropy.inc")) if not l.startswith("//")))]
assert len(ENT) == 128


def _table(name):
    text = open(os.path.join(_PKG, "host", "cabac_tables.hpp")).read()
    m = re.search(name + r"\[\d+\]\s*=\s*\{([^}]*)\}", text)
    return [int(x) for x in re.findall(r"\d+", m.group(1))]


SIG8, LAST8 = _table("cabac_sig8x8"), _table("cabac_last8x8")
assert len(SIG8) == 63 and len(LAST8) == 63
TRANS_LPS = [0, 0, 1, 2, 2, 4, 4, 5, 6, 7, 8, 9, 9, 11, 11, 12, 13, 13, 15, 15, 16, 16, 18, 18, 19, 19, 21, 21, 22, 22, 23, 24,
             24, 25, 26, 26, 27, 27, 28, 29, 29, 30, 30, 30, 31, 32, 32, 33, 33, 33, 34, 34, 35, 35, 35, 36, 36, 36, 37, 37, 37, 38, 38, 63]
S4 = [[13107, 8066, 5243], [11916, 7490, 4660], [10082, 6554, 4194], [9362, 5825, 3647], [8192, 5243, 3355], [7282, 4559, 2893]]
S8 = [[13107, 11428, 20972, 12222, 16777, 15481], [11916, 10826, 19174, 11058, 14980, 14290], [10082, 8943, 15978, 9675, 12710, 11985],
      [9362, 8228, 14913, 8931, 11984, 11259], [8192, 7346, 13159, 7740, 10486, 9777], [7282, 6428, 11570, 6830, 9118, 8640]]
CLS8 = [[0, 3, 4, 3], [3, 1, 5, 1], [4, 5, 2, 5], [3, 1, 5, 1]]
ZZ4 = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]
_fix8 = lambda x: int(x * 256 + 0.5)
W2_4 = [_fix8(3.125), _fix8(1.25), _fix8(0.5)]                                           # coef_weight2: the inverse squared norms of the basis functions
W2_8 = [_fix8(x) for x in (1.00000, 0.78487, 2.56132, 0.88637, 1.60040, 1.41850)]
W1_4 = [_fix8(x) for x in (1.76777, 1.11803, 0.70711)]                                   # coef_weight1: their square roots, the same class order
W1_8 = [_fix8(x) for x in (1.0000, 0.8859, 1.6000, 0.9415, 1.2651, 1.1910)]
SIG_OFF, LAST_OFF, ABS_OFF = [105, 120, 134, 149, 152, 402], [166, 181, 195, 210, 213, 417], [227, 237, 247, 257, 266, 426]
SCORE_MAX, SCORE_BIAS = 1 << 200, 1 << 60                                                # (Python integers: the bias only keeps the arithmetic x264's)


def zigzag8():
    zz, r, c, up = [], 0, 0, True
    for _ in range(64):
        zz.append(r * 8 + c)
        if up:
            if c == 7: r += 1; up = False
            elif r == 0: c += 1; up = False
            else: r -= 1; c += 1
        else:
            if r == 7: c += 1; up = True
            elif c == 0: r += 1; up = True
            else: r += 1; c -= 1
    return zz


ZZ8 = zigzag8()


def ncoef(cat):
    return 64 if cat == 5 else 4 if cat == 3 else 16


def zigzag(cat):
    return ZZ8 if cat == 5 else list(range(4)) if cat == 3 else ZZ4


def psy_q8(f_psy_trellis):
    """i_psy_trellis of a session: (int)(f_psy_trellis / 4 * 256 + 0.5)"""
    return int(f_psy_trellis / 4 * 256 + 0.5)


def _srd(x, s):
    return x << -s if s <= 0 else (x + (1 << (s - 1))) >> s


def scan_tables(cat, qp):
    """quantiser, rounding offset, inverse, coef_weight2 and coef_weight1 of every scan position (flat matrices)"""
    nc, zz, dc = ncoef(cat), zigzag(cat), cat in (0, 3)
    mf, bias, unq, w2, w1 = [], [], [], [], []
    for i in range(nc):
        if dc:
            m0 = _srd(S4[qp % 6][0], qp // 6 - 1)
            mf.append(m0 >> 1); bias.append(((1 << 15) // m0) << 1); unq.append(((1 << (qp // 6 + 15 + 8)) // S4[qp % 6][0]) << 1); w2.append(256); w1.append(256)
        elif cat == 5:
            cl = CLS8[(zz[i] >> 3) & 3][zz[i] & 3]
            m = _srd(S8[qp % 6][cl], qp // 6)
            mf.append(m); bias.append((1 << 15) // m); unq.append((1 << (qp // 6 + 16 + 8)) // S8[qp % 6][cl]); w2.append(W2_8[cl]); w1.append(W1_8[cl])
        else:
            cl = (zz[i] & 1) + ((zz[i] >> 2) & 1)
            m = _srd(S4[qp % 6][cl], qp // 6 - 1)
            mf.append(m); bias.append((1 << 15) // m); unq.append((1 << (qp // 6 + 15 + 8)) // S4[qp % 6][cl]); w2.append(W2_4[cl]); w1.append(W1_4[cl])
    return mf, bias, unq, w2, w1


def mf_raster(cat, qp):
    """the quantiser row oracle/quant.c hands x264o_quant_trellis_cabac (flat matrices), raster order"""
    mf = scan_tables(1 if cat in (0, 3) else cat, qp)[0]
    out, zz = [0] * len(mf), zigzag(1 if cat in (0, 3) else cat)
    for i, m in enumerate(mf):
        out[zz[i]] = m
    return out


def lambda2(intra, qp):
    return int((0.65 * 0.65 if intra else 0.85 * 0.85) * 2.0 ** (qp / 3.0 + 6.0) + 0.5)


def ent(st, b):
    return ENT[st ^ b]


def trans(st, b):
    s, mps = st >> 1, st & 1
    if mps ^ b:
        return (TRANS_LPS[s] << 1) | ((mps ^ 1) if s == 0 else mps)
    return (min(s + 1, 62) << 1) | mps


def _unary():
    su, tu = [[0] * 128 for _ in range(15)], [[0] * 128 for _ in range(15)]
    for prefix in range(15):
        for c0 in range(128):
            bits, ctx = 0, c0
            for _ in range(1, prefix):
                bits += ent(ctx, 1); ctx = trans(ctx, 1)
            if 0 < prefix < 14:
                bits += ent(ctx, 0); ctx = trans(ctx, 0)
            su[prefix][c0] = bits + 256; tu[prefix][c0] = ctx
    return su, tu


SIZE_UNARY, TRANS_UNARY = _unary()


def size_ue_big(v):
    return 2 * ((v + 1).bit_length() - 1) + 1


def _sign(v, s):
    return -v if s < 0 else v


class _Node:
    __slots__ = ("score", "levels", "cs")

    def __init__(self):
        self.score, self.levels, self.cs = SCORE_MAX, (), [0, 0, 0, 0]


def quant_trellis(coefs, cat, qp, intra, states, psy=0, fenc=None):
    """coefs: one block's signed transform coefficients in scan order (AC categories: 16 entries, entry 0 ignored); states: the slice's 460 context
    variables; psy: i_psy_trellis; fenc: the source block's transform in the same order (read where psy applies).  Returns the levels in scan order."""
    nc, b_ac, dc, chroma = ncoef(cat), int(cat in (1, 4)), cat in (0, 3), cat in (3, 4)
    mf, bias, unq, w2, w1 = scan_tables(cat, qp)
    lam = lambda2(intra, qp)
    sig, last, cabac_state = states[SIG_OFF[cat]:], states[LAST_OFF[cat]:], [int(x) for x in states[ABS_OFF[cat]:ABS_OFF[cat] + 10]]
    lg_last = 8 if chroma and dc else 9
    orig = [int(c) for c in coefs]
    if b_ac:
        orig[0] = 0
    quant = [((bias[i] + abs(orig[i])) * mf[i]) >> 16 for i in range(nc)]
    if not any(quant):
        return [0] * nc
    last_nnz = nc - 1
    while last_nnz > b_ac and not quant[last_nnz]:
        last_nnz -= 1
    sigidx = (lambda i: SIG8[i]) if cat == 5 else (lambda i: i - b_ac)
    lastidx = (lambda i: LAST8[i]) if cat == 5 else (lambda i: i - b_ac)
    use_psy = bool(psy) and not dc and not chroma

    def distortion(i, c, unquant_abs):
        """what every node but the first pays for reconstructing |c| as unquant_abs"""
        d = abs(c) - unquant_abs
        ssd = d * d * w2[i]
        if use_psy and i:
            pred = int(fenc[i]) - c
            ssd -= w1[i] * psy * abs(unquant_abs + _sign(pred, c))
        return ssd

    if last_nnz == 0 and not dc:
        cost_sig = ent(int(sig[0]), 1) + ent(int(last[0]), 1)
        c, q = orig[0], quant[0]
        bscore, ret = SCORE_MAX, 0
        for lvl in (q - 1, q):
            ua = (unq[0] * lvl + 128) >> 8
            d = c - ((_sign(ua, c) + 8) & ~15)
            score = d * d * w2[0]
            if lvl:
                prefix = min(lvl - 1, 14)
                f8 = cost_sig + ent(cabac_state[1], int(prefix > 0)) + SIZE_UNARY[prefix][cabac_state[5]]
                if lvl >= 15:
                    f8 += size_ue_big(lvl - 15) << 8
                score += (f8 * lam) >> 4
            if score < bscore:
                bscore, ret = score, lvl
        return [_sign(ret, c)] + [0] * (nc - 1)

    level_state = cabac_state + [0, 0]
    init4 = [cabac_state[0], cabac_state[4], cabac_state[8], cabac_state[9]]
    cur = [_Node() for _ in range(8)]
    cur[0].score = SCORE_BIAS
    live = lambda n: n.score < SCORE_MAX
    ctx_hi = 0
    for i in range(last_nnz, b_ac - 1, -1):
        q = quant[i]
        if not q:
            if not ctx_hi:
                cur[0].score -= (ent(int(sig[sigidx(i)]), 0) * lam) >> 4
            for j in range(1, 8 if ctx_hi else 4):
                if live(cur[j]):
                    cur[j].levels = (0,) + cur[j].levels
            continue
        c = orig[i]
        prev, cur = cur, [_Node() for _ in range(8)]
        for j in range(ctx_hi):                       # (nodes below ctx_hi keep what they had: dead in ctx_hi)
            cur[j] = prev[j]
        if i < nc - 1:
            s1 = ent(int(sig[sigidx(i)]), 1)
            siglast = [ent(int(sig[sigidx(i)]), 0), ent(int(last[lastidx(i)]), 0) + s1, ent(int(last[lastidx(i)]), 1) + s1]
        else:
            siglast = [0, 0, 0]
        ssd0, ssd1 = [0, 0], [0, 0]
        for k in range(2):
            lvl = q - 1 + k
            ua = (unq[i] * lvl + 128) >> 8
            ssd1[k] = distortion(i, c, ua)
            ssd0[k] = ssd1[k]
            if i == 0 and not dc and not ctx_hi:
                d = c - ((_sign(ua, c) + 8) & ~15)
                ssd0[k] = d * d * w2[i]

        def coef(j, const_level, lvl, node_ctx, level1_ctx, levelgt1_ctx, ssd):
            score = prev[j].score + ssd
            f8 = siglast[1 if j else 2]
            l1s = prev[j].cs[level1_ctx >> 2] if j >= 3 else level_state[level1_ctx]
            f8 += ent(l1s, int(const_level > 1))
            lgs, prefix = 0, min(lvl - 1, 14)
            if const_level > 1:
                lgs = prev[j].cs[levelgt1_ctx - 6] if j >= 6 else level_state[levelgt1_ctx]
                f8 += SIZE_UNARY[prefix][lgs] + ((size_ue_big(lvl - 15) << 8) if lvl >= 15 else 0)
            else:
                f8 += 256
            score += (f8 * lam) >> 4
            dst = cur[node_ctx]
            if score < dst.score:
                dst.score = score
                if j == 2 or (j <= 3 and node_ctx == 4):
                    dst.cs = init4[:]
                elif j >= 3:
                    dst.cs = prev[j].cs[:]
                if j >= 3:
                    dst.cs[level1_ctx >> 2] = trans(l1s, int(const_level > 1))
                if const_level > 1 and node_ctx == 7:
                    dst.cs[levelgt1_ctx - 6] = TRANS_UNARY[prefix][lgs]
                dst.levels = (lvl,) + prev[j].levels

        def coef0(s0):
            if not ctx_hi:
                cur[0].score = prev[0].score + s0; cur[0].levels = prev[0].levels
                for j in range(1, 4):
                    if not live(prev[j]):
                        break
                    cur[j].score = prev[j].score; cur[j].cs = prev[j].cs[:]; cur[j].levels = (0,) + prev[j].levels
            else:
                for j in range(1, 8):
                    if live(prev[j]):
                        cur[j].score = prev[j].score; cur[j].cs = prev[j].cs[:]; cur[j].levels = (0,) + prev[j].levels

        def coef1(s0, s1_):
            to, l1 = [1, 2, 3, 3, 4, 5, 6, 7], [1, 2, 3, 4, 0, 0, 0, 0]
            for j in range(ctx_hi, 8 if ctx_hi else 4):
                if not j or live(prev[j]):
                    coef(j, 1, 1, to[j], l1[j], 0, s1_ if j else s0)
                elif not ctx_hi:
                    return

        def coefn(lvl, s0, s1_):
            to, l1, lg = [4, 4, 4, 4, 5, 6, 7, 7], [1, 2, 3, 4, 0, 0, 0, 0], [5, 5, 5, 5, 6, 7, 8, 9]
            for j in range(ctx_hi, 8 if ctx_hi else 4):
                if not j or live(prev[j]):
                    coef(j, 2, lvl, to[j], l1[j], lg_last if j == 7 else lg[j], s1_ if j else s0)
                elif not ctx_hi:
                    return

        if q == 1:
            ssd1[0] += (siglast[0] * lam) >> 4
            coef0(ssd0[0] - ssd1[0])
            coef1(ssd0[1] - ssd1[0], ssd1[1] - ssd1[0])
        elif q == 2:
            coef1(ssd0[0], ssd1[0])
            coefn(q, ssd0[1], ssd1[1])
            ctx_hi = 1
        else:
            coefn(q - 1, ssd0[0], ssd1[0])
            coefn(q, ssd0[1], ssd1[1])
            ctx_hi = 1
    best = ctx_hi
    for j in range(ctx_hi + 1, 8 if ctx_hi else 4):
        if cur[j].score < cur[best].score:
            best = j
    out = [0] * nc
    if best == 0:
        return out
    lv = cur[best].levels                              # (a path that left node 0 at position i has nothing above i: zeros)
    lv = lv + (0,) * (last_nnz - b_ac + 1 - len(lv))
    for k, i in enumerate(range(b_ac, last_nnz + 1)):
        out[i] = _sign(lv[k], orig[i])
    return out


def quant_trellis_blocks(coefs_scan, cat, qp, intra, states, psy=0, fenc_scan=None):
    """every row of coefs_scan through quant_trellis: (levels, non-zero flags) as numpy arrays"""
    import numpy as np
    out = np.zeros_like(coefs_scan)
    for b in range(len(coefs_scan)):
        out[b] = quant_trellis(coefs_scan[b].tolist(), cat, qp, intra, states, psy, None if fenc_scan is None else fenc_scan[b].tolist())
    return out, (out != 0).any(axis=1).astype(np.uint8)


def random_blocks(cat, qp, kind, nblk, rng):
    """random blocks in scan order: dense (Laplacian amplitudes of a few quantiser steps), sparse (every guess 0 or 1), zero (below half a step: every
    guess 0), escape (levels of 15 and more)"""
    import numpy as np
    nc = ncoef(cat)
    mf = np.array(scan_tables(cat, qp)[0], np.float64)
    step = 65536.0 / mf
    if kind == "dense":
        c = rng.laplace(0.0, 1.0, (nblk, nc)) * step[None, :] * (3.0 / (1.0 + 0.3 * np.arange(nc)))[None, :] * rng.choice([0.5, 1.0, 3.0], (nblk, 1))
    elif kind == "sparse":
        c = rng.uniform(0.6, 1.4, (nblk, nc)) * step[None, :] * (rng.random((nblk, nc)) < rng.choice([0.1, 0.3, 1.0], (nblk, 1))) * rng.choice([-1, 1], (nblk, nc))
        c[0] = 0; c[0, 1 if cat in (1, 4) else 0] = 1.2 * step[0]            # nothing but the first coefficient: the DC-only shortcut
    elif kind == "zero":
        c = rng.uniform(-0.45, 0.45, (nblk, nc)) * step[None, :]
    else:
        c = rng.laplace(0.0, 1.0, (nblk, nc)) * step[None, :] * 1.5
        for b in range(nblk):
            for i in rng.choice(nc, 2, replace=False):
                c[b, i] = rng.choice([-1, 1]) * step[i] * rng.choice([15.2, 16.0, 17.6, 31.0, 47.3, 200.0])
    c = np.clip(np.trunc(c), -32000, 32000).astype(np.int16)
    if cat in (1, 4):
        c[:, 0] = 0
    return c


def random_states(rng):
    import numpy as np
    return ((rng.integers(0, 63, 460) << 1) | rng.integers(0, 2, 460)).astype(np.uint8)

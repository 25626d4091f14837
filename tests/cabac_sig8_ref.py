"""Serial restatement of the residual coding of ONE 8x8 luma block (ctxBlockCat 5) as the CABAC pricing runs it: the significance map bin by bin on the 15
significant_coeff_flag and 9 last_significant_coeff_flag contexts that the block's positions share (which position sees which context: the generated
csrc/cabac_masks8x8.inc), then the levels (cabac_levels_ref.block_levels) — in both orders the device knows: "stream", 7.3.5.3.3's (positions upwards), and
"size", x264's size-only coder's (from the last coefficient down).  The checker of the device's 8x8 maps as per-context strings in the level walk
(csrc/cabac_rd.hip.h cab_levels_all, primitive x264gpu_cabac_residual_walk).  Test infrastructure: pure Python."""
import os
import re

from cabac_levels_ref import LV_CHROMA_AC, LV_CHROMA_DC, MB_LEVELS, _block, block_levels, step

_HERE = os.path.dirname(os.path.abspath(__file__))
_MASKS = [int(x, 16) for x in re.findall(r"0x([0-9a-fA-F]{16})ull", open(os.path.join(_HERE, "..", "x264vfw_amd", "csrc", "cabac_masks8x8.inc")).read())]
assert len(_MASKS) == 24
SIG_CTX, LAST_CTX = [None] * 63, [None] * 63          # position -> context (position 63 has neither)
for _c, _m in enumerate(_MASKS):
    for _p in range(64):
        if (_m >> _p) & 1:
            _t = SIG_CTX if _c < 15 else LAST_CTX
            assert _p < 63 and _t[_p] is None
            _t[_p] = _c if _c < 15 else _c - 15
assert None not in SIG_CTX and None not in LAST_CTX
MAP_OFF, MAP_SIZE, MAP_STREAM = 0, 1, 2               # csrc/cabac_rd.hip.h CAB_MAP8_*
SIG_LANE0, LAST_LANE0, ABS_LANE0 = 0, 16, 32          # where the contexts sit in the role-indexed register r8 (csrc/cabac_layout.hip.h)


def map_bins(coefs, order):
    """the significance map's bins of a block (64 coefficients in scan order, at least one non-zero) in coding order: (role, context, bin), role 0 =
    significant_coeff_flag, 1 = last_significant_coeff_flag"""
    lastp = max(p for p in range(64) if coefs[p])
    top = min(lastp, 62)                              # position 63 is never coded: a block that reaches it ends there by inference
    out = []
    for p in (range(top, -1, -1) if order == MAP_SIZE else range(top + 1)):
        out.append((0, SIG_CTX[p], 1 if coefs[p] else 0))
        if coefs[p]:
            out.append((1, LAST_CTX[p], 1 if p == lastp else 0))
    return out


def block8(coefs, r8, bits, order):
    """one 8x8 block on the role-indexed register r8 (a list of 64 context variables, updated): the map in the given order (none for MAP_OFF), then the levels"""
    if order != MAP_OFF:
        for role, c, b in map_bins(coefs, order):
            lane = (LAST_LANE0 if role else SIG_LANE0) + c
            r8[lane], co = step(r8[lane], b); bits += co
    ctx = [r8[ABS_LANE0 + i] for i in range(10)]
    bits = block_levels(coefs, ctx, bits)
    for i in range(10): r8[ABS_LANE0 + i] = ctx[i]
    return bits


def mb_coefs8(lv, b):
    """the 64 coefficients of 8x8 block b in scan order out of a macroblock's levels (x264gpu_mb layout: position p lies in 4x4 group p & 3 at p >> 2)"""
    return [lv[(b * 4 + (p & 3)) * 16 + (p >> 2)] for p in range(64)]


def put_coefs8(lv, b, coefs):
    for p in range(64): lv[(b * 4 + (p & 3)) * 16 + (p >> 2)] = coefs[p]


def case(lv, nz0, order, r, r8, nzdc=0, nzac=0):
    """a macroblock with 8x8 transform: the luma blocks of mask nz0 (each must hold a coefficient), then the chroma DC planes of nzdc and the chroma AC blocks of
    nzac as cabac_levels_ref codes them -> (what[6], expected r, expected r8, expected bits)"""
    r0, r80, bits = [x[:] for x in r], r8[:], 0
    for b in range(4):
        if (nz0 >> b) & 1:
            bits = block8(mb_coefs8(lv, b), r80, bits, order)
    for pl in range(2):
        if (nzdc >> pl) & 1:
            bits = _block(lv[LV_CHROMA_DC + pl * 4:LV_CHROMA_DC + pl * 4 + 4], r0, 3, 48, 52, 55, 9, bits)
    for b in range(8):
        if (nzac >> b) & 1:
            bits = _block(lv[LV_CHROMA_AC + b * 16 + 1:LV_CHROMA_AC + b * 16 + 16], r0, 2, 0, 16, 32, 10, bits)
    return [5 if nz0 else -1, nz0, nzac, nzdc, 0, order], r0, r80, bits


def random_block(rnd, dens, scale):
    co = [0 if rnd.random() > dens else rnd.choice([-1, 1]) * max(1, int(abs(rnd.gauss(0, scale)))) for _ in range(64)]
    if not any(co): co[rnd.randrange(64)] = rnd.choice([-1, 1])
    if rnd.random() < 0.5:                            # as real blocks are: nothing above some position
        cut = rnd.randrange(64)
        co = co[:cut + 1] + [0] * (63 - cut)
        if not any(co): co[cut] = 1
    return co


def random_case(rnd):
    lv = [0] * MB_LEVELS
    nz0 = rnd.randrange(1, 16)
    dens, scale = rnd.random() ** 2, rnd.choice([1, 1, 2, 4, 20, 60])
    for b in range(4):                                # (blocks outside the mask hold levels too: they must not be coded)
        put_coefs8(lv, b, random_block(rnd, dens, scale))
    nzdc = nzac = 0
    if rnd.random() < 0.5:
        for i in range(8): lv[LV_CHROMA_DC + i] = rnd.randint(-3, 3)
        for i in range(128): lv[LV_CHROMA_AC + i] = 0 if rnd.random() > 0.3 else rnd.randint(-4, 4)
        nzdc = sum(1 << pl for pl in range(2) if any(lv[LV_CHROMA_DC + pl * 4:LV_CHROMA_DC + pl * 4 + 4]))
        nzac = sum(1 << b for b in range(8) if any(lv[LV_CHROMA_AC + b * 16 + 1:LV_CHROMA_AC + b * 16 + 16]) and rnd.random() < 0.8)
    r = [[rnd.randrange(126) for _ in range(4)] for _ in range(64)]
    r8 = [rnd.randrange(126) for _ in range(64)]
    order = rnd.choice([MAP_SIZE, MAP_SIZE, MAP_STREAM, MAP_STREAM, MAP_OFF])
    return (lv, r, r8) + tuple(case(lv, nz0, order, r, r8, nzdc, nzac))

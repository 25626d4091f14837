"""The restatement the device's 8x8 significance-map strings are checked against (tests/cabac_sig8_ref.py) agrees with a straight coding of the block by the
standard: 7.3.5.3.3's loop over the positions in scan order with Table 9-43's ctxIdxInc of frame-coded 8x8 blocks typed out here, and 9.3.4.2's state machine.
The descending (size) order sends every context the same bins reversed.  No GPU."""
import random

import cabac_sig8_ref as R8
from cabac_levels_ref import block_levels, step

# Table 9-43, frame coded blocks with ctxBlockCat 5: ctxIdxInc of significant_coeff_flag and last_significant_coeff_flag by levelListIdx (0..62)
SIG8 = [0, 1, 2, 3, 4, 5, 5, 4, 4, 3, 3, 4, 4, 4, 5, 5, 4, 4, 4, 4, 3, 3, 6, 7, 7, 7, 8, 9, 10, 9, 8, 7,
        7, 6, 11, 12, 13, 11, 6, 7, 8, 9, 14, 10, 9, 8, 6, 11, 12, 13, 11, 6, 9, 14, 10, 9, 11, 12, 13, 11, 14, 10, 12]
LAST8 = [0] + [1] * 15 + [2] * 16 + [3] * 8 + [4] * 8 + [5] * 4 + [6] * 4 + [7] * 4 + [8] * 3


def straight(coefs, sig, last, ctx, bits):
    """residual_block_cabac of an 8x8 block: numCoeff = 64, the map position by position until the last coefficient, then the levels from the last one down"""
    num = 64
    i, seen_last = 0, False
    while i < num - 1:
        s = 1 if coefs[i] else 0
        sig[SIG8[i]], co = step(sig[SIG8[i]], s); bits += co
        if s:
            l = 0 if any(coefs[i + 1:]) else 1
            last[LAST8[i]], co = step(last[LAST8[i]], l); bits += co
            if l:
                seen_last = True
                break
        i += 1
    assert seen_last or coefs[63]
    return block_levels(coefs, ctx, bits)


def _blocks():
    rnd = random.Random(0x518)
    out = [[1] + [0] * 63, [0] * 62 + [3, 0], [0] * 63 + [-2], [7] * 64, [1] * 64, [0] * 16 + [2] * 16 + [0] * 32, [0] * 16 + [2] * 16 + [0] * 8 + [1] + [0] * 23,
           [1] + [0] * 4 + [-1] + [0] * 58, [20] * 40 + [0] * 24]
    for _ in range(400):
        out.append(R8.random_block(rnd, rnd.random() ** 2, rnd.choice([1, 2, 4, 20])))
    return out


def test_tables_agree_with_the_generated_masks():
    assert len(SIG8) == 63 and len(LAST8) == 63
    assert R8.SIG_CTX == SIG8 and R8.LAST_CTX == LAST8


def test_stream_order_equals_straight_coding():
    rnd = random.Random(5)
    for co in _blocks():
        r8 = [rnd.randrange(126) for _ in range(64)]
        want = r8[:]
        sig, last, ctx = want[0:15], want[16:25], want[32:42]
        wbits = straight(co, sig, last, ctx, 0)
        want[0:15], want[16:25], want[32:42] = sig, last, ctx
        got = r8[:]
        gbits = R8.block8(co, got, 0, R8.MAP_STREAM)
        assert got == want and gbits == wbits, co


def test_size_order_reverses_every_contexts_bins():
    for co in _blocks():
        per = {}
        for order in (R8.MAP_STREAM, R8.MAP_SIZE):
            for role, c, b in R8.map_bins(co, order):
                per.setdefault((order, role, c), []).append(b)
        keys = {k[1:] for k in per}
        for k in keys:
            assert per[(R8.MAP_SIZE,) + k] == per[(R8.MAP_STREAM,) + k][::-1], (co, k)
        # and a `last` context's string is all zero but for the block's last position, where it is coded at all
        lastp = max(p for p in range(64) if co[p])
        ones = sum(sum(v) for k, v in per.items() if k[0] == R8.MAP_STREAM and k[1] == 1)
        assert ones == (1 if lastp < 63 else 0)


def test_map_off_is_levels_only():
    rnd = random.Random(6)
    for co in _blocks()[:50]:
        r8 = [rnd.randrange(126) for _ in range(64)]
        got = r8[:]
        bits = R8.block8(co, got, 0, R8.MAP_OFF)
        ctx = r8[32:42]
        assert bits == block_levels(co, ctx, 0) and got[32:42] == ctx and got[:32] == r8[:32] and got[42:] == r8[42:]

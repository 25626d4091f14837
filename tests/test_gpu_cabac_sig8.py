"""The 8x8 luma blocks' significance maps as per-context bit strings in the level walk (csrc/cabac_rd.hip.h cab_levels_all with CabLv::map8: lanes 0..14 / 16..24
of r8 compact their context's bins out of the word's non-zero mask and walk them beside the level contexts) through the primitive
x264gpu_cabac_residual_walk, against the bin-by-bin restatement tests/cabac_sig8_ref.py: same bits, every byte of r / r8 the same, in both orders."""
import random

import numpy as np
import pytest

import cabac_sig8_ref as R8
from cabac_levels_ref import LV_CHROMA_AC, LV_CHROMA_DC, MB_LEVELS

pytestmark = pytest.mark.gpu


def _pack(rows):
    return np.array([[b[0] | (b[1] << 8) | (b[2] << 16) | (b[3] << 24) for b in r] for r in rows], np.uint32)


def _run(lib, fn, lv, what, r, r8):
    import torch
    n = len(lv)
    d = lambda a: torch.from_numpy(np.ascontiguousarray(a)).cuda()
    d_lv, d_w = d(np.array(lv, np.int16)), d(np.array(what, np.int32))
    d_r, d_r8 = d(_pack(r).view(np.int32)), d(np.array(r8, np.uint32).view(np.int32))
    d_ro, d_r8o, d_b = torch.zeros_like(d_r), torch.zeros_like(d_r8), torch.zeros(n, dtype=torch.int32, device="cuda")
    lib.check(fn(d_lv.data_ptr(), d_w.data_ptr(), n, d_r.data_ptr(), d_r8.data_ptr(), d_ro.data_ptr(), d_r8o.data_ptr(), d_b.data_ptr(), None), "cabac walk")
    torch.cuda.synchronize()
    return d_b.cpu().numpy(), d_ro.cpu().numpy().view(np.uint32), d_r8o.cpu().numpy().view(np.uint32)


def _check(lib, cases, names=None):
    """cases: (lv, r, r8, what6, r_want, r8_want, bits_want)"""
    got_b, got_r, got_r8 = _run(lib, lib.x264gpu_cabac_residual_walk, [c[0] for c in cases], [c[3] for c in cases], [c[1] for c in cases], [c[2] for c in cases])
    for i, c in enumerate(cases):
        tag = (names[i] if names else i, c[3])
        assert got_b[i] == c[6], ("bits", tag, int(got_b[i]), c[6])
        assert (got_r8[i] == np.array(c[5], np.uint32)).all(), ("r8", tag, np.nonzero(got_r8[i] != np.array(c[5], np.uint32))[0].tolist())
        assert (got_r[i] == _pack([c[4]])[0]).all(), ("r", tag)


def test_residual_walk_random_cases_vs_serial_restatement(gpu):
    rnd = random.Random(0x8158)
    cases = [R8.random_case(rnd) for _ in range(600)]
    _check(gpu, cases)
    orders = [c[3][5] for c in cases]
    assert min(orders.count(o) for o in (R8.MAP_OFF, R8.MAP_SIZE, R8.MAP_STREAM)) > 60 and max(c[6] for c in cases) > 100000          # the cases are not trivial


def _fixed_blocks():
    """name -> the 64 coefficients (scan order) of an edge-case block"""
    lone = lambda p, v=1: [v if i == p else 0 for i in range(64)]
    out = {
        "single coefficient at 0 (the only member of last context 0)": lone(0),
        "single coefficient at 62": lone(62, -1),
        "single coefficient at 63 (never coded: no last flag at all)": lone(63, 2),
        "all 64 non-zero": [(-1) ** i * (1 + i % 3) for i in range(64)],
        "last position the only member of last context 1": [3] + [0] * 8 + [1] + [0] * 54,
        "last position the only member of last context 8": [1, 0, -1] + [0] * 58 + [1, 0, 0],
        "16 positions in last context 2, ending there": [0] * 16 + [1, -1] * 8 + [0] * 32,
        "16 positions in last context 2, last beyond": [1] + [0] * 15 + [2, -1] * 8 + [0] * 9 + [1] + [0] * 22,
        "escape levels": [15, -16, 14, 200, 0, 0, -2047, 1, 31, 0, 15] + [0] * 53,
        "cg string beyond 63 bins (serial fallback beside the map)": [9] * 40 + [0] * 24,
        "cg string beyond 63 bins, escapes": [(-1) ** i * 40 for i in range(64)],
    }
    return out


@pytest.mark.parametrize("order", [R8.MAP_SIZE, R8.MAP_STREAM])
def test_residual_walk_edge_blocks(gpu, order):
    rnd = random.Random(77 + order)
    cases, names = [], []
    for name, co in _fixed_blocks().items():
        for b in range(4):                                   # the block in each place of the macroblock, its neighbours full of levels that are not coded
            lv = [rnd.randint(-2, 2) for _ in range(MB_LEVELS)]
            R8.put_coefs8(lv, b, co)
            r, r8 = [[rnd.randrange(126) for _ in range(4)] for _ in range(64)], [rnd.randrange(126) for _ in range(64)]
            cases.append((lv, r, r8) + tuple(R8.case(lv, 1 << b, order, r, r8)))
            names.append(name)
    _check(gpu, cases, names)


@pytest.mark.parametrize("order", [R8.MAP_SIZE, R8.MAP_STREAM])
def test_residual_walk_block_masks(gpu, order):
    """part mode's one or two blocks and the whole macroblock: the blocks of the mask in order, on the contexts the earlier ones left"""
    rnd = random.Random(99 + order)
    cases, names = [], []
    for mask in (1, 2, 4, 8, 5, 10, 15):
        for dens in (0.05, 0.4, 1.0):
            lv = [0] * MB_LEVELS
            for b in range(4): R8.put_coefs8(lv, b, R8.random_block(rnd, dens, 3))
            r, r8 = [[rnd.randrange(126) for _ in range(4)] for _ in range(64)], [rnd.randrange(126) for _ in range(64)]
            cases.append((lv, r, r8) + tuple(R8.case(lv, mask, order, r, r8)))
            names.append("mask %d" % mask)
    _check(gpu, cases, names)


def test_map_off_equals_the_level_walk(gpu):
    """category 5 with the map off is x264gpu_cabac_level_walk's contract: levels only"""
    rnd = random.Random(3)
    lvs, whats, rs, r8s = [], [], [], []
    for _ in range(40):
        lv = [0] * MB_LEVELS
        for b in range(4): R8.put_coefs8(lv, b, R8.random_block(rnd, rnd.random(), rnd.choice([1, 4, 30])))
        for i in range(8): lv[LV_CHROMA_DC + i] = rnd.randint(-2, 2)
        for i in range(128): lv[LV_CHROMA_AC + i] = rnd.randint(-1, 1)
        nzdc = sum(1 << pl for pl in range(2) if any(lv[LV_CHROMA_DC + pl * 4:LV_CHROMA_DC + pl * 4 + 4]))
        nzac = sum(1 << b for b in range(8) if any(lv[LV_CHROMA_AC + b * 16 + 1:LV_CHROMA_AC + b * 16 + 16]))
        lvs.append(lv); whats.append([5, rnd.randrange(1, 16), nzac, nzdc, 0])
        rs.append([[rnd.randrange(126) for _ in range(4)] for _ in range(64)]); r8s.append([rnd.randrange(126) for _ in range(64)])
    a = _run(gpu, gpu.x264gpu_cabac_level_walk, lvs, whats, rs, r8s)
    b = _run(gpu, gpu.x264gpu_cabac_residual_walk, lvs, [w + [R8.MAP_OFF] for w in whats], rs, r8s)
    for x, y in zip(a, b):
        assert np.array_equal(x, y)
    assert a[0].min() > 0
    # and it is what the restatement says
    cases = [(lv, r, r8) + tuple(R8.case(lv, w[1], R8.MAP_OFF, r, r8, w[3], w[2])) for lv, w, r, r8 in zip(lvs, whats, rs, r8s)]
    _check(gpu, cases)

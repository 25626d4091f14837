"""The two loops of the trellis quantiser (csrc/trellis.hip.h) and the test that chooses between them, through x264gpu_trellis_blocks_ex: the
levels-of-one loop (a call whose round-to-nearest guesses are all 0 or 1) and the general loop.  Whichever runs, levels and non-zero flags are those of
oracle/trellis.cpp; d_paths says which ran (one byte per pass of eight blocks: bit 0 = levels-of-one; bit 1, 32-bit scores, is never set: no loop on
narrower scores is built)."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O

pytestmark = pytest.mark.gpu

S4 = [[13107, 8066, 5243], [11916, 7490, 4660], [10082, 6554, 4194], [9362, 5825, 3647], [8192, 5243, 3355], [7282, 4559, 2893]]
S8 = [[13107, 11428, 20972, 12222, 16777, 15481], [11916, 10826, 19174, 11058, 14980, 14290], [10082, 8943, 15978, 9675, 12710, 11985],
      [9362, 8228, 14913, 8931, 11984, 11259], [8192, 7346, 13159, 7740, 10486, 9777], [7282, 6428, 11570, 6830, 9118, 8640]]
CLS8 = [[0, 3, 4, 3], [3, 1, 5, 1], [4, 5, 2, 5], [3, 1, 5, 1]]
ZZ4 = [0, 1, 4, 8, 5, 2, 3, 6, 9, 12, 13, 10, 7, 11, 14, 15]


def _zigzag8():
    zz8 = np.zeros(64, np.int64)
    r, c_, up = 0, 0, True
    for i in range(64):                       # frame zigzag of an 8x8 block
        zz8[i] = r * 8 + c_
        if up:
            if c_ == 7: r += 1; up = False
            elif r == 0: c_ += 1; up = False
            else: r -= 1; c_ += 1
        else:
            if r == 7: c_ += 1; up = True
            elif c_ == 0: r += 1; up = True
            else: r += 1; c_ -= 1
    return zz8


def _ncoef(cat):
    return 64 if cat == 5 else 4 if cat == 3 else 16


def _zz(cat):
    return _zigzag8() if cat == 5 else np.arange(4) if cat == 3 else np.array(ZZ4)


def _mf(cat, qp):
    """the quantiser row as oracle/quant.c builds it (flat matrices), in raster order"""
    shr = lambda x, s: x << -s if s <= 0 else (x + (1 << (s - 1))) >> s
    if cat == 5:
        return np.array([shr(S8[qp % 6][CLS8[(i >> 3) & 3][i & 3]], qp // 6) for i in range(64)], np.uint16)
    return np.array([shr(S4[qp % 6][(i & 1) + ((i >> 2) & 1)], qp // 6 - 1) for i in range(16)], np.uint16)


def _mf_scan(cat, qp):
    """quantiser and rounding offset of every scan position, as the search's guess uses them (DC categories: mf[0] >> 1, the offset doubled)"""
    mf = _mf(cat, qp).astype(np.int64)
    nc = _ncoef(cat)
    if cat in (0, 3):
        return np.full(nc, mf[0] >> 1), np.full(nc, ((1 << 15) // mf[0]) << 1)
    m = mf[_zz(cat)]
    return m, (1 << 15) // m


def _guess(cat, qp, coefs_scan):
    m, bias = _mf_scan(cat, qp)
    g = ((bias[None, :] + np.abs(coefs_scan.astype(np.int64))) * m[None, :]) >> 16
    if cat in (1, 4):
        g[:, 0] = 0
    return g


def _states(rng):
    return ((rng.integers(0, 63, 460) << 1) | rng.integers(0, 2, 460)).astype(np.uint8)


def _oracle(cat, qp, intra, coefs_scan, states):
    """levels and non-zero flags of oracle/trellis.cpp, block by block"""
    O.L.x264o_quant_trellis_cabac.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
    O.L.x264o_quant_trellis_cabac.restype = C.c_int
    nc, zz, mf = _ncoef(cat), _zz(cat), _mf(cat, qp)
    want = np.zeros_like(coefs_scan)
    want_nz = np.zeros(len(coefs_scan), np.uint8)
    for b in range(len(coefs_scan)):
        raster = np.zeros(nc, np.int16)
        raster[zz] = coefs_scan[b]
        want_nz[b] = O.L.x264o_quant_trellis_cabac(raster.ctypes.data, mf.ctypes.data, qp, cat, intra, states.ctypes.data) != 0
        want[b] = raster[zz]
    return want, want_nz


def _device(lib, cat, qp, intra, coefs_scan, states, force_general=0):
    import torch
    nblk = len(coefs_scan)
    d_c, d_s = torch.from_numpy(coefs_scan.copy()).cuda(), torch.from_numpy(states).cuda()
    d_l, d_z = torch.zeros_like(d_c), torch.zeros(nblk, dtype=torch.uint8, device="cuda")
    d_p = torch.full(((nblk + 7) // 8,), 0xff, dtype=torch.uint8, device="cuda")
    lib.check(lib.x264gpu_trellis_blocks_ex(d_c.data_ptr(), nblk, cat, qp, intra, d_s.data_ptr(), d_l.data_ptr(), d_z.data_ptr(), force_general, d_p.data_ptr(), None),
              "trellis_blocks_ex")
    torch.cuda.synchronize()
    return d_l.cpu().numpy(), d_z.cpu().numpy(), d_p.cpu().numpy()


def _same(got, got_nz, want, want_nz, coefs_scan):
    bad = np.nonzero((got != want).any(axis=1))[0]
    assert len(bad) == 0, (f"{len(bad)} of {len(want)} blocks differ; first {bad[0]}: coefs {coefs_scan[bad[0]].tolist()} device {got[bad[0]].tolist()} "
                           f"oracle {want[bad[0]].tolist()}")
    np.testing.assert_array_equal(got_nz, want_nz)


def _ones_blocks(cat, qp, nblk, seed):
    """blocks whose every coefficient is 0 or +- a value whose guess is 1: magnitudes of 0.6 to 1.4 quantiser steps of their position, a density that
    varies from block to block (some full), an empty block and one with nothing but its first coefficient"""
    rng = np.random.default_rng(seed)
    nc = _ncoef(cat)
    m, _ = _mf_scan(cat, qp)
    step = 65536.0 / m
    mag = np.ceil(rng.uniform(0.6, 1.4, (nblk, nc)) * step[None, :] - 1e-9)
    mag = np.minimum(mag, np.floor(1.4 * step[None, :]))
    density = rng.choice([0.05, 0.2, 0.5, 1.0], (nblk, 1))
    keep = rng.random((nblk, nc)) < density
    coefs = (mag * keep * rng.choice([-1, 1], (nblk, nc))).astype(np.int16)
    first = 1 if cat in (1, 4) else 0
    if cat in (1, 4):
        coefs[:, 0] = 0
    coefs[0] = 0                                        # an empty block
    coefs[1] = 0; coefs[1, first] = int(mag[1, first])  # only the first coefficient
    coefs[9] = 0; coefs[9, first] = -int(mag[9, first])
    for p in range(nblk // 8):                          # (every pass of eight blocks has something to search)
        if not coefs[8 * p + 3, first]:
            coefs[8 * p + 3, first] = int(mag[8 * p + 3, first])
    return coefs


@pytest.mark.parametrize("nblk", [208, 203])
@pytest.mark.parametrize("qp,intra", [(20, 1), (23, 0), (25, 0), (30, 0), (44, 0), (51, 1)])
@pytest.mark.parametrize("cat", [0, 1, 2, 3, 4, 5])
def test_all_ones_takes_the_levels_of_one_loop(gpu, cat, qp, intra, nblk):
    """every guess is 0 or 1 (26 full passes of eight blocks, or a short last pass): every pass runs the levels-of-one loop, and the levels are the
    oracle's"""
    coefs = _ones_blocks(cat, qp, 208, 7000 + 10 * cat + qp)[:nblk]
    g = _guess(cat, qp, coefs)
    assert g.max() == 1
    states = _states(np.random.default_rng(100 * cat + qp))
    want, want_nz = _oracle(cat, qp, intra, coefs, states)
    got, got_nz, paths = _device(gpu, cat, qp, intra, coefs, states)
    _same(got, got_nz, want, want_nz, coefs)
    assert len(paths) == 26
    assert (paths == 1).all(), f"passes without the levels-of-one loop: {np.nonzero(paths != 1)[0].tolist()}"
    assert np.count_nonzero(want) > nblk // 4          # the cases are not trivial


@pytest.mark.parametrize("qp,intra", [(20, 1), (23, 0), (25, 0), (30, 0)])
@pytest.mark.parametrize("cat", [0, 1, 2, 3, 4, 5])
def test_one_big_level_per_pass_takes_the_general_loop(gpu, cat, qp, intra):
    """the same blocks with one coefficient per pass of eight raised to a guess of 2: no pass may run the levels-of-one loop"""
    nblk = 208
    coefs = _ones_blocks(cat, qp, nblk, 7000 + 10 * cat + qp)
    m, _ = _mf_scan(cat, qp)
    nc = _ncoef(cat)
    rng = np.random.default_rng(31 * cat + qp)
    for p in range(nblk // 8):
        b, i = 8 * p + int(rng.integers(0, 8)), int(rng.integers(1 if cat in (1, 4) else 0, nc))
        coefs[b, i] = int(np.ceil(2.0 * 65536.0 / m[i])) * (-1 if p & 1 else 1)
    g = _guess(cat, qp, coefs)
    assert g.max() == 2 and all(g[8 * p:8 * p + 8].max() == 2 for p in range(nblk // 8))
    states = _states(np.random.default_rng(100 * cat + qp))
    want, want_nz = _oracle(cat, qp, intra, coefs, states)
    got, got_nz, paths = _device(gpu, cat, qp, intra, coefs, states)
    _same(got, got_nz, want, want_nz, coefs)
    assert not (paths & 1).any(), f"passes in the levels-of-one loop: {np.nonzero(paths & 1)[0].tolist()}"


def _natural_blocks(cat, qp, intra, nblk=203):
    """the coefficient distribution of test_gpu_prims.py::test_trellis_primitive_vs_oracle: Laplacian amplitudes falling with frequency, a share of
    blocks nearly empty, a few with big levels"""
    rng = np.random.default_rng(1000 * cat + qp + intra)
    nc = _ncoef(cat)
    step = 65536.0 / float(_mf(cat, qp)[0])
    amp = step * (2.5 / (1.0 + 0.35 * np.arange(nc)))
    coefs = (rng.laplace(0.0, 1.0, (nblk, nc)) * amp * rng.choice([0.15, 0.6, 1.0, 3.0, 12.0], (nblk, 1))).astype(np.int64)
    coefs = np.clip(coefs, -30000, 30000).astype(np.int16)
    first = 1 if cat in (1, 4) else 0
    if cat in (1, 4):
        coefs[:, 0] = 0
    coefs[0] = 0
    coefs[1] = 0; coefs[1, first] = int(step * 1.4)
    return coefs, _states(rng)


@pytest.mark.parametrize("huge", [0, 1])
@pytest.mark.parametrize("intra", [0, 1])
@pytest.mark.parametrize("qp", [8, 20, 23, 30, 37, 44, 51])
@pytest.mark.parametrize("cat", [2, 5])
def test_quantiser_sweep_with_huge_coefficients(gpu, cat, qp, intra, huge):
    """natural blocks over the quantiser range, inter and intra, with and without a few coefficients at +-30000 (levels in the thousands at qp 8): the
    oracle's levels.  Scores are 64 bits wide in every loop, so no pass may report 32-bit scores (bit 1), and a pass that holds a +-30000 coefficient
    cannot be a levels-of-one pass"""
    coefs, states = _natural_blocks(cat, qp, intra)
    big_passes = []
    if huge:
        rng = np.random.default_rng(77 + cat + qp)
        for b in (5, 42, 43, 120, 202):
            coefs[b, int(rng.integers(0, 3))] = 30000 if b & 1 else -30000
            big_passes.append(b // 8)
    want, want_nz = _oracle(cat, qp, intra, coefs, states)
    got, got_nz, paths = _device(gpu, cat, qp, intra, coefs, states)
    _same(got, got_nz, want, want_nz, coefs)
    assert (paths <= 1).all()
    assert not paths[big_passes].any()
    # bit 0 is exact: set in the passes whose guesses are all 0 or 1, and in no other
    g = _guess(cat, qp, coefs)
    expect = np.array([0 < g[8 * p:8 * p + 8].max() <= 1 for p in range(len(paths))])
    np.testing.assert_array_equal(paths & 1, expect.astype(np.uint8))


@pytest.mark.parametrize("qp,intra", [(23, 0), (20, 1), (8, 0), (37, 1), (51, 0), (30, 0)])
@pytest.mark.parametrize("cat", [0, 1, 2, 3, 4, 5])
def test_forced_general_equals_automatic(gpu, cat, qp, intra):
    """the inputs of test_trellis_primitive_vs_oracle through the hook: the general loop on 64-bit scores alone and the automatic choice give the
    same bytes, and the forced call reports no other loop"""
    coefs, states = _natural_blocks(cat, qp, intra)
    a_lv, a_nz, a_paths = _device(gpu, cat, qp, intra, coefs, states, force_general=0)
    f_lv, f_nz, f_paths = _device(gpu, cat, qp, intra, coefs, states, force_general=1)
    assert a_lv.tobytes() == f_lv.tobytes() and a_nz.tobytes() == f_nz.tobytes()
    assert (f_paths == 0).all() and (a_paths <= 1).all()

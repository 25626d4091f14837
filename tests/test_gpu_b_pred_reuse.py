"""GPU: the B slices' prediction memo (k_mb.hip.h PMEMO: the direct prediction and both lists' 16x16 winners' rows are fetched once a macroblock and
the candidate encodes that ask for the same rows again are served from registers).  Same comparison as test_gpu_bframes.run — records, levels,
reconstruction and CABAC context variables against the CPU checker picture by picture, the stream decoded back — on content chosen so that the memo
can go wrong: each case first asserts, on the CHECKER's records alone, that its content reaches the path it is there for."""
import functools

import numpy as np
import pytest

import bgop
import oracle_lib as O
from synth import synth_frames
from test_gpu_bframes import MEDIUM, run

pytestmark = pytest.mark.gpu


# ---- content ----
def _texture(rng, h, w, lo, hi, cell=4):
    """band-limited texture: random values on a coarse grid, enlarged and smoothed with a 3x3 box"""
    g = rng.integers(lo, hi, ((h + cell - 1) // cell + 1, (w + cell - 1) // cell + 1)).astype(np.float64)
    t = np.kron(g, np.ones((cell, cell)))[:h, :w]
    p = np.pad(t, 1, mode="edge")
    return sum(p[dy:dy + h, dx:dx + w] for dy in range(3) for dx in range(3)) / 9.0


def pan_frames(w, h, n, seed, dx, dy, noise):
    """a texture translated by (dx, dy) pixels a frame (chroma sampled from full-resolution planes: half that), +-noise per luma sample, +-2 on chroma"""
    rng = np.random.default_rng(seed)
    mx, my = abs(dx) * n, abs(dy) * n
    H, W = h + my + 2, w + mx + 2
    Y, U, V = _texture(rng, H, W, 16, 236), _texture(rng, H, W, 90, 150, 8), _texture(rng, H, W, 100, 160, 8)
    frames = []
    for t in range(n):
        ox, oy = (mx - dx * t) if dx > 0 else -dx * t, (my - dy * t) if dy > 0 else -dy * t
        y = Y[oy:oy + h, ox:ox + w] + rng.integers(-noise, noise + 1, (h, w))
        u = U[oy:oy + h:2, ox:ox + w:2] + rng.integers(-2, 3, (h // 2, w // 2))
        v = V[oy:oy + h:2, ox:ox + w:2] + rng.integers(-2, 3, (h // 2, w // 2))
        frames.append(np.concatenate([np.clip(np.rint(p), 16, 235).astype(np.uint8).ravel() for p in (y, u, v)]))
    return frames


def static_frames(w, h, n, seed, noise):
    """one picture of the project's synthetic content, fresh noise of +-noise on every frame's luma (+-1 on chroma)"""
    rng = np.random.default_rng(seed)
    base = synth_frames(w, h, 1, seed=seed)[0].astype(np.int32)
    amp = np.concatenate([np.full(w * h, noise), np.full(w * h // 2, 1)])
    return [np.clip(base + rng.integers(-amp, amp + 1), 16, 235).astype(np.uint8) for _ in range(n)]


# ---- what the checker decides on that content (CPU only; once per content and configuration) ----
@functools.lru_cache(maxsize=None)
def _oracle_b_records(content, w, h, types, seed, pyramid, direct, over):
    from x264vfw_amd import host_api as HL
    kw = dict(MEDIUM, **dict(over))
    cfg = O.default_config(w, h, **kw)
    out = []
    order = bgop.encode_gop(HL, O.OracleEncoder(cfg), content(w, h, len(types), seed), types, cfg, 20, 23, 25, kw["refs"], 3, pyramid, 0, out, None, direct)[2]
    recs = [e[1] for e in out if e[0] != "direct"]
    assert len(recs) == len(order)
    return [(disp, m) for (disp, pt), m in zip(order, recs) if pt >= 3]


def _stats(content, w, h, types, seed, pyramid=1, direct="spatial", **over):
    mbw = (w + 15) // 16
    s = dict(bi=0, same_left=0, bi_odd=0, bi_zero=0, direct=0, skip=0, inter=0)
    for disp, m in _oracle_b_records(content, w, h, types, seed, pyramid, direct, tuple(sorted(over.items()))):
        ty, r0, r1, v0, v1 = m["type"], m["ref"][:, 0], O.mb_ref1(m)[:, 0], m["mv"][:, 0], O.mb_mv1(m)[:, 0]
        inter = ty == O.MB_B_INTER
        bi = inter & (r0 >= 0) & (r1 >= 0)
        s["bi"] += int(bi.sum())
        s["bi_odd"] += int(bi.sum()) if disp % 4 != 2 else 0          # (without the pyramid: pictures nearer to one reference than to the other)
        s["bi_zero"] += int((bi & ~v0.any(axis=1) & ~v1.any(axis=1)).sum())
        l0 = inter & (r0 >= 0) & v0.any(axis=1)
        same = l0[1:] & l0[:-1] & (r0[1:] == r0[:-1]) & (v0[1:] == v0[:-1]).all(axis=1) & (np.arange(1, len(ty)) % mbw != 0)
        s["same_left"] += int(same.sum())
        s["direct"] += int((ty == O.MB_B_DIRECT).sum())
        s["skip"] += int((ty == O.MB_B_SKIP).sum())
        s["inter"] += int((inter | (ty == O.MB_B_8x8)).sum())
    return s


def noisy_pan(w, h, n, seed):
    return pan_frames(w, h, n, seed, 2, -1, 14)


def static_noise(w, h, n, seed):
    return static_frames(w, h, n, seed, 6)


def fast_pan(w, h, n, seed):
    return pan_frames(w, h, n, seed, 9, 6, 6)


# ---- 1. noisy global pan: BI combined from held rows, the bidirectional refinement moving vectors after the fill, neighbours with equal vectors ----
def test_noisy_pan_bi_from_held_rows(gpu):
    st = _stats(noisy_pan, 96, 80, "IBBBPBBBP", 1)
    print(st)
    assert st["bi"] >= 20 and st["same_left"] >= 5, st
    run(gpu, 96, 80, "IBBBPBBBP", 1, frames=noisy_pan(96, 80, 9, 1))


def test_noisy_pan_without_pyramid_weights_not_32(gpu):
    st = _stats(noisy_pan, 96, 80, "IBBBPBBBP", 1, pyramid=0)
    print(st)
    assert st["bi_odd"] >= 10, st
    run(gpu, 96, 80, "IBBBPBBBP", 1, pyramid=0, frames=noisy_pan(96, 80, 9, 1))


@pytest.mark.parametrize("seed", [2, 3, 4])
def test_noisy_pan_three_streams(gpu, seed):
    st = _stats(noisy_pan, 96, 80, "IBBBPBBBP", seed)
    print(st)
    assert st["bi"] >= 20, st
    run(gpu, 96, 80, "IBBBPBBBP", seed, streams=3, frames=noisy_pan(96, 80, 9, seed))


# ---- 2. static picture, fresh noise per frame: B_DIRECT / B_SKIP from held direct rows, bi-prediction at zero vectors (the zero-vector probe) ----
@pytest.mark.parametrize("direct", ["spatial", "temporal", "auto"])
def test_static_noise_direct_and_skip_from_held_rows(gpu, direct):
    st = _stats(static_noise, 96, 80, "IBBBPBBBP", 5, direct=direct)
    print(st)
    if direct == "spatial":
        assert st["direct"] >= 30 and st["skip"] >= 10 and st["bi_zero"] >= 3, st
    else:
        assert st["direct"] + st["skip"] >= 10, st
    run(gpu, 96, 80, "IBBBPBBBP", 5, direct=direct, frames=static_noise(96, 80, 9, 5))


# ---- 3. fast pan on a picture of a few macroblocks: vectors at the mv_min / mv_max clamp (keys on unclamped vectors, fetches on clamped ones) ----
def test_fast_pan_vectors_at_the_clamp(gpu):
    st = _stats(fast_pan, 48, 32, "IBBBPBBP", 6)
    print(st)
    assert st["inter"] >= 5, st
    run(gpu, 48, 32, "IBBBPBBP", 6, frames=fast_pan(48, 32, 8, 6))


# ---- 4. content 1 through the other B instantiations ----
@pytest.mark.parametrize("over", [
    dict(subme=9, rd=63),                                           # RD refinement: b_predict with the coroutine's own vectors, no memo
    dict(rd=0, trellis=0, subme=5, psy=0, psy_rd_q8=0),             # no RD: the quarter-pel refinement moves the winners after the fill
    dict(cabac=0, trellis=0),
    dict(me_method=2),
    dict(me_method=0),
], ids=["rdrefine", "nord", "cavlc", "umh", "dia"])
def test_noisy_pan_other_instantiations(gpu, over):
    st = _stats(noisy_pan, 64, 48, "IBBBP", 7, **over)
    print(st)
    assert st["inter"] >= 5, st
    run(gpu, 64, 48, "IBBBP", 7, frames=noisy_pan(64, 48, 5, 7), **over)


# ---- 5. slices: one wavefront each, each with its own memo (x264's slice threads want four macroblock rows a slice: twelve rows for three) ----
def test_noisy_pan_three_slices(gpu):
    st = _stats(noisy_pan, 96, 192, "IBBBPBBBP", 8, slices=3)
    print(st)
    assert st["bi"] >= 20, st
    run(gpu, 96, 192, "IBBBPBBBP", 8, frames=noisy_pan(96, 192, 9, 8), slices=3)

"""Test content: a band-limited texture under a global pan (the generator tests/test_gpu_b_pred_reuse.py introduced, here as a module other tests can
import).  Deterministic in its arguments; luma clipped to [16, 235]."""
import numpy as np


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

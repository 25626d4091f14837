"""Full-range and saturated test pictures, and the one table of cases that tests/test_hard_content_cpu.py (what the checker reaches on them) and
tests/test_gpu_hard_content.py (device == checker on them) both run.

Every other picture generator of the suite clips luma to [16, 235] and chroma to [16, 240]; on that content the checker's largest level is about
300 and no reconstructed sample ever sits at 0 or 255.  The kinds below hand the encoder what an application may hand a VfW codec: samples over
the whole of 0..255, pictures made of 0 and 255 alone, flat pictures at both rails.  Each generator is `(w, h, n, seed) -> [I420 uint8 array] * n`
and deterministic in its arguments."""
import numpy as np


def _i420(y, u, v):
    return np.concatenate([np.ascontiguousarray(p, np.uint8).ravel() for p in (y, u, v)])


def _planes(f, w, h):
    """views of the Y, U and V planes of an I420 array"""
    n, c = w * h, (w // 2) * (h // 2)
    return f[:n].reshape(h, w), f[n:n + c].reshape(h // 2, w // 2), f[n + c:].reshape(h // 2, w // 2)


def _cells(rng, h, w, cell):
    """h x w samples of 0 / 255, constant over cell x cell blocks"""
    g = rng.integers(0, 2, ((h + cell - 1) // cell, (w + cell - 1) // cell), dtype=np.uint8) * 255
    return np.kron(g, np.ones((cell, cell), np.uint8))[:h, :w]


def noise_full(w, h, n, seed):
    """every sample of the three planes uniform over 0..255, fresh per frame"""
    rng = np.random.default_rng(seed)
    return [rng.integers(0, 256, w * h * 3 // 2, dtype=np.uint8) for _ in range(n)]


def binary_cells(cell, static=False):
    """random 0 / 255 per cell x cell block on all planes, V = 255 - U; fresh per frame, or (static) one picture with ~2 % of its luma samples
    flipped afresh in every frame: skips and direct macroblocks next to the largest residuals there are"""
    def gen(w, h, n, seed):
        rng = np.random.default_rng(seed)
        out = []
        y = u = None
        for _ in range(n):
            if y is None or not static:
                y, u = _cells(rng, h, w, cell), _cells(rng, h // 2, w // 2, cell)
            yy = y ^ ((rng.random((h, w)) < 0.02).astype(np.uint8) * 255) if static else y
            out.append(_i420(yy, u, 255 - u))
        return out
    gen.__name__ = f"cells{cell}" + ("_static" if static else "")
    return gen


def checker(period):
    """0 / 255 checkerboard of that period, moving one sample to the left a frame (period 1: inverted every frame): all the energy in single
    high-frequency coefficients, the largest residual at zero motion"""
    def gen(w, h, n, seed):
        def board(hh, ww, t):
            yy, xx = np.mgrid[0:hh, 0:ww]
            return ((((xx + t + seed) // period + yy // period) & 1) * 255).astype(np.uint8)
        out = []
        for t in range(n):
            u = board(h // 2, w // 2, t)
            out.append(_i420(board(h, w, t), u, 255 - u))
        return out
    gen.__name__ = f"checker{period}"
    return gen


def flash(w, h, n, seed):
    """whole pictures alternately all 0 and all 255, chroma too: flat macroblocks, DC prediction at the rails, the largest SAD at every candidate"""
    return [np.full(w * h * 3 // 2, 255 * ((t + seed) & 1), np.uint8) for t in range(n)]


def moving_edges(w, h, n, seed):
    """random 0 / 255 blocks of 8x8 cut from a larger canvas at (7, 5) samples a frame: the edges leave the transform grid, the vectors run to the
    picture's border"""
    rng = np.random.default_rng(seed)
    H, W = h + 5 * n + 8, w + 7 * n + 8
    Y, U = _cells(rng, H, W, 8), _cells(rng, H // 2, W // 2, 8)
    out = []
    for t in range(n):
        oy, ox = 5 * t, 7 * t
        u = U[oy // 2:oy // 2 + h // 2, ox // 2:ox // 2 + w // 2]
        out.append(_i420(Y[oy:oy + h, ox:ox + w], u, 255 - u))
    return out


def rails_ramp(w, h, n, seed):
    """a horizontal 0..255 ramp in luma, a vertical one in chroma (V falling), +-3 of noise clipped at 0 / 255: full range without saturation"""
    rng = np.random.default_rng(seed)
    yy, xx = np.mgrid[0:h, 0:w]
    cy = np.mgrid[0:h // 2, 0:w // 2][0]
    y0, u0 = xx * 255 // (w - 1), cy * 255 // (h // 2 - 1)
    out = []
    for _ in range(n):
        f = lambda p, s: np.clip(p + rng.integers(-3, 4, s), 0, 255)
        out.append(_i420(f(y0, (h, w)), f(u0, u0.shape), f(255 - u0, u0.shape)))
    return out


KINDS = {g.__name__: g for g in [noise_full] + [binary_cells(c, s) for s in (False, True) for c in (1, 2, 4, 8)] + [checker(p) for p in (1, 2, 4)]
         + [flash, moving_edges, rails_ramp]}
BINARY = [k for k in KINDS if k not in ("noise_full", "rails_ramp")]          # the kinds made of 0 and 255 alone
MID_QP = 30                                                                   # "up to mid quantisers" of the rail condition

# the four picture sizes: two plain ones and the two ragged ones (neither dimension a multiple of 16)
SIZES = [(64, 48), (96, 80), (64, 48), (70, 38), (64, 48), (50, 58)]


def _size(i):
    return SIZES[i % len(SIZES)]


# ---- a. I / P pipeline (x264gpu_encode_frames): an IDR first and again at picture 3 ----
CABAC_RD = dict(cabac=1, rd=1, subme=7, psy=1, psy_rd_q8=256, partitions=7, dct8x8=1)
MEDIUM_IP = dict(CABAC_RD, refs=3, mixed_refs=1, chroma_me=1)
IP_CONFIGS = {
    "cavlc_q0": dict(qp_i=0, qp_p=0, partitions=3, refs=2),
    "cavlc_q4": dict(qp_i=4, qp_p=2, partitions=7, dct8x8=1, dct_decimate=0),
    "cavlc_q51": dict(qp_i=51, qp_p=51),
    "cavlc_rd_q10": dict(qp_i=10, qp_p=12, rd=1, subme=6, partitions=7, dct8x8=1),
    "cabac_rd_q0": dict(CABAC_RD, qp_i=0, qp_p=1, trellis=63),
    "cabac_rd_q24": dict(MEDIUM_IP, qp_i=24, qp_p=26, trellis=127, chroma_qp_offset=-2),
    "cabac_rd_q51": dict(CABAC_RD, qp_i=51, qp_p=51, trellis=63),
}


def big_levels(kind, qmax, rd):
    """the I / P cases designated to reach |level| > 2047.  At quantisers 0 / 1: content whose 4x4 blocks are flat at a rail (the energy of 16 luma
    DC coefficients meets in the DC transform of an Intra_16x16 macroblock — which the decision without RD does not choose on flat pictures, hence
    flash with RD only — or in the DC of a block whose prediction sits at the other rail); the period-1 and period-2 checkerboards spread theirs
    over smaller multipliers (1004 - 2345).  At quantiser 4 the largest level there is is 3264 x 0.625 = 2040, so of the 4 / 2 configuration only
    the P pictures (quantiser 2: 2510) can pass the mark, and do where fresh flat blocks meet a prediction at the other rail: cells of 8."""
    return (qmax <= 1 and (kind in ("checker4", "moving_edges") or (kind == "flash" and bool(rd)))) or (qmax <= 4 and kind in ("cells8", "cells8_static"))


def big_cost(kind, qmax, rd, size=None):
    """the I / P cases designated to reach a record cost > 2^20: quantiser 51 with RD (the cost is then SSD + lambda2 x bits; without RD it is a SATD
    score, bounded by about 6 x 10^4 for 8-bit samples) on every kind but the flat pictures, which code for next to nothing (5.6 x 10^5), and the
    ramp at all sizes but the narrowest, where it is steepest (1.08 x 10^6; 0.77 - 1.00 x 10^6 at the others)"""
    return qmax == 51 and bool(rd) and kind != "flash" and (kind != "rails_ramp" or size == (50, 58))


def _ip(name, kind, w, h, kw, n=5, seed=1):
    qmax = max(kw["qp_i"], kw["qp_p"])
    return dict(id=f"{name}-{kind}-{w}x{h}", kind=kind, w=w, h=h, n=n, seed=seed, kw=kw, big_levels=big_levels(kind, qmax, kw.get("rd")),
                big_cost=big_cost(kind, qmax, kw.get("rd"), (w, h)))


def _ip_cases():
    out = []
    for ci, (name, kw) in enumerate(IP_CONFIGS.items()):
        for ki, kind in enumerate(KINDS):
            w, h = _size(ci + ki)
            out.append(_ip(name, kind, w, h, kw, seed=10 + ki))
    out.append(_ip("cabac_rd_q51", "rails_ramp", 50, 58, IP_CONFIGS["cabac_rd_q51"], seed=24))          # the ramp at its steepest: a cost beyond 2^20
    for kind in ("flash", "moving_edges", "cells8"):          # RD on CAVLC bit counts with levels beyond 2047: the long escape of the level codes
        out.append(_ip("cavlc_rd_q0", kind, 64, 48, dict(qp_i=0, qp_p=0, rd=1, subme=6, partitions=7, dct8x8=1), seed=3))
    for name, me in (("dia", dict(me_method=0)), ("umh", dict(me_method=2)), ("umh32", dict(me_method=2, me_range=32)), ("esa", dict(me_method=3))):
        for kind in ("noise_full", "moving_edges"):
            for qp in (26, 51):
                out.append(_ip(f"{name}_q{qp}", kind, 96, 80, dict(dict(me_range=16, partitions=3, refs=2, qp_i=qp, qp_p=qp), **me), n=4, seed=3))
    for st in (0.51985, 1.55955):
        for kind, (w, h) in (("flash", (64, 48)), ("cells8", (70, 38)), ("rails_ramp", (96, 80))):
            out.append(_ip(f"aq{st:.1f}", kind, w, h, dict(aq_mode=1, aq_strength=st, partitions=7, dct8x8=1, qp_i=24, qp_p=27), seed=5))
    for rd in (63, 63 | 64):
        for me in (1, 2):
            for kind in ("checker2", "moving_edges", "cells4_static"):
                for qi, qp in ((0, 1), (28, 30)):
                    kw = dict(MEDIUM_IP, subme=8, rd=rd, me_method=me, trellis=63, refs=2, qp_i=qi, qp_p=qp)
                    out.append(_ip(f"refine{rd}_me{me}_q{qi}", kind, 64, 48, kw, n=4, seed=7))
    for kind in ("noise_full", "checker1"):
        for qp in (20, 37):
            out.append(_ip(f"psytrellis_q{qp}", kind, 64, 48, dict(MEDIUM_IP, trellis=127, psy_trellis_q8=38, chroma_qp_offset=-2, qp_i=qp, qp_p=qp), n=4, seed=9))
    for plain in (0, 1):          # (x264's slice threads want four macroblock rows a slice: 64x192 for three of them; --slices 3 at 64x96)
        out.append(_ip("slices3" + "_plain" * plain, "moving_edges", 64, 96 if plain else 192, dict(MEDIUM_IP, slices=3, slices_plain=plain, trellis=63, qp_i=22, qp_p=25), n=4, seed=11))
    return out


IP_CASES = _ip_cases()
# one lock-step batch of four streams, each with its own kind of content
MULTI = dict(w=64, h=48, n=4, seed=13, kinds=("noise_full", "flash", "moving_edges", "cells2_static"), kw=dict(MEDIUM_IP, trellis=63, qp_i=18, qp_p=21))


# ---- b. B pictures (test_gpu_bframes.run with frames=): every kind at three quantiser triples, the structures and toolsets dealt round ----
SLOW_B = dict(me_method=2, trellis=127, subme=9, rd=63 | 64)
B_QPS = ((0, 1, 2), (20, 23, 25), (49, 51, 51))
# scale / denom / offset of the P pictures of "IBPBBP" over flash(seed=1) (display 0, 2: all 255 outside the patches; 5: all 0): picture 2 predicts 255 from 255 as
# 255 x 127 / 64 = 506, clipped to 255; picture 5 predicts 0 from 255 as 255 / 4 - 128 = -64, clipped to 0
FLASH_WEIGHTS = {2: (127, 6, 0), 5: (1, 2, -128)}


B_PATCH_MBS = ((0, 0), (1, 0), (0, 1), (1, 1), (2, 0), (3, 0))          # the macroblocks (x, y) that b_patches writes into


def _implicit_w1(tb, td):
    """the weight (of 64) that implicit weighted bi-prediction gives list 1's reference: tb pictures after list 0's, td between the two"""
    return ((tb * ((16384 + td // 2) // td) + 32) >> 6) >> 2


def b_patches(frames, w, h, types, seed):
    """The pictures of a B case: the kind's own, with three patches of 32x16 samples in the top left corner that make every B picture hold the
    three families of macroblock types whatever the kind and the quantiser (a saturated picture by itself mostly offers the B analysis one thing).
    - (0, 0) a cross-fade in opposite motion: every I / P picture shows 0 / 255 cells of 8 of its own; a B picture shows its earlier neighbour's,
      moved left by 2 samples a picture, blended with its later neighbour's, moved left towards it, in the weights of implicit weighted
      bi-prediction.  Only both lists together, each with a vector of its own, predict its first macroblock: bi-predicted inter.
    - (0, 16) the first picture's samples in every picture: direct or skipped.
    - (32, 0) in B pictures horizontal stripes of 0 / 255, 4 rows each, another order in every picture: no reference has them, horizontal intra
      prediction does."""
    rng = np.random.default_rng(seed + 1000)
    anchors = [t for t, c in enumerate(types) if c != "B"]
    cy = {a: _cells(rng, 16, 48, 8).astype(np.int32) for a in anchors}
    cu = {a: _cells(rng, 8, 24, 4).astype(np.int32) for a in anchors}
    first = [p.copy() for p in _planes(frames[0], w, h)]
    out = []
    for t, f in enumerate(frames):
        y, u, v = (p.copy() for p in _planes(f, w, h))
        if t in anchors:
            py, pu, pv = cy[t][:, :32], cu[t][:, :16], 255 - cu[t][:, :16]
        else:
            a0, a1 = max(a for a in anchors if a < t), min(a for a in anchors if a > t)
            w1 = _implicit_w1(t - a0, a1 - a0)
            s0, s1 = 2 * (t - a0), 2 * (a1 - t)
            mix = lambda p, q: (p * (64 - w1) + q * w1 + 32) >> 6
            py = mix(cy[a0][:, s0:s0 + 32], cy[a1][:, s1:s1 + 32])
            pu = mix(cu[a0][:, s0 // 2:s0 // 2 + 16], cu[a1][:, s1 // 2:s1 // 2 + 16])
            pv = mix(255 - cu[a0][:, s0 // 2:s0 // 2 + 16], 255 - cu[a1][:, s1 // 2:s1 // 2 + 16])
            code = (t * 5 + 3) % 14 + 1                                      # four stripes, never all alike, another order in every picture
            sy = np.array([255 * (code >> (r // 4) & 1) for r in range(16)], np.uint8)[:, None]
            y[0:16, 32:64], u[0:8, 16:32], v[0:8, 16:32] = sy, sy[::2], 255 - sy[::2]
        y[0:16, 0:32], u[0:8, 0:16], v[0:8, 0:16] = py, pu, pv
        y[16:32, 0:32], u[8:16, 0:16], v[8:16, 0:16] = first[0][16:32, 0:32], first[1][8:16, 0:16], first[2][8:16, 0:16]
        out.append(_i420(y, u, v))
    return out


def _b_cases():
    out = []
    i = 0
    for ki, kind in enumerate(KINDS):
        for qi, qps in enumerate(B_QPS):
            w, h = _size(i)
            over = dict(SLOW_B) if (ki + qi) % 3 == 2 else {}          # slow's toolset at every quantiser triple in turn
            c = dict(kind=kind, w=w, h=h, types=("IBBBPBBP", "IBPBBP")[i % 2], seed=20 + ki, qps=qps, pyramid=(i // 2) % 2 ^ 1,
                     direct=("spatial", "temporal", "auto")[(i // 3 + i) % 3], weightp=0, weights=None, over=over)
            c["big_levels"], c["big_cost"] = qps[0] == 0, max(qps) == 51          # (with the patches every kind reaches both marks)
            c["id"] = f"{kind}-q{qps[0]}-{c['types']}-{w}x{h}-{c['direct']}-pyr{c['pyramid']}" + ("-slow" if over else "")
            out.append(c)
            i += 1
    out.append(dict(id="noise_full-weightp2", kind="noise_full", w=64, h=48, types="IBPBBPP", seed=41, qps=B_QPS[1], pyramid=1, direct="spatial", weightp=2, weights=None, over={}, big_levels=False, big_cost=False))
    out.append(dict(id="flash-explicit-weights", kind="flash", w=64, h=48, types="IBPBBP", seed=1, qps=B_QPS[1], pyramid=1, direct="spatial", weightp=2,
                    weights=FLASH_WEIGHTS, over={}, big_levels=False, big_cost=False))
    return out


B_CASES = _b_cases()

# ---- c. lookahead ----
LA_SIZES = ((80, 48), (32, 32))
LA_FRAMES = 4
LA_W, LA_H = LA_SIZES[0]
SLICETYPE_KINDS = ("cells4_static", "checker2", "noise_full")
# the macroblock-tree walks: (kind, picture types, seed); the last is long and static enough for the propagate cost to saturate at 32767 (the
# checker takes 0.02 s over it)
MBTREE_CASES = [(k, "PBBBPBBBP", 33) for k in SLICETYPE_KINDS] + [("cells2_static", "P" + "BBBP" * 10, 33)]


# ---- what the checker makes of a case (CPU only) ----
def frames_of(case):
    n = case.get("n") or len(case["types"])
    frames = KINDS[case["kind"]](case["w"], case["h"], n, case["seed"])
    return b_patches(frames, case["w"], case["h"], case["types"], case["seed"]) if "types" in case else frames


def ip_slice_type(i):
    return 2 if i in (0, 3) else 0


def rail_share(recons):
    a = np.concatenate(recons)
    return float(((a == 0) | (a == 255)).mean())

"""GPU: the Intra_4x4 analysis in ten anti-diagonal rounds of two blocks (csrc/k_mb.hip.h mb_analyse_intra: one U build, one prediction + SATD pass, one
transform / quantiser / inverse for both blocks of a round; the exit from the rounds on partial sums) and the paired predictor build of the final
encode (mb_encode_i4x4_trellis).  Whole pictures against the CPU checker — records, levels, reconstruction and the CABAC context variables after every
picture (the comparisons of test_gpu_pipeline.compare and test_gpu_bframes.run) — on content whose noise sweeps the loop's exit threshold: each case
first asserts, on the CHECKER's records alone, that its content reaches the path it is there for.  The checker exposes no exit index, so the amplitude
sweeps (and the random one at the end) are the coverage of the exit.  (The RD-refinement instantiations — the subme 8 / 9 routes below with rd=63 — keep the
loop in coding order: same cases, same comparison.)"""
import functools
import random

import numpy as np
import pytest

import oracle_lib as O
from synth import synth_frames
from test_gpu_bframes import MEDIUM, run
from test_gpu_cabac_header import IP, _b_records, _ip_records, ip_run
from test_gpu_pipeline import CABAC_CTX_I, CABAC_CTX_P, compare

pytestmark = pytest.mark.gpu

MB_I4x4 = 0          # x264gpu_mb.type of an Intra_4x4 macroblock


def shift_noise(w, h, n, seed, amp):
    """a picture panning two columns a frame under fresh noise of +-amp: inter prediction is left with the noise, so amp moves the intra analysis'
    thresholds (min(inter, i16, i8) x 9 / 8 under RD) across the Intra_4x4 costs"""
    base = synth_frames(w, h, 1, seed=seed)[0]
    y0, uv = base[:w * h].reshape(h, w).astype(np.int64), base[w * h:]
    rng = np.random.default_rng(seed)
    out = []
    for t in range(n):
        y = np.roll(y0, 2 * t, axis=1) + rng.integers(-amp, amp + 1, (h, w))
        out.append(np.concatenate([np.clip(y, 16, 235).astype(np.uint8).ravel(), uv]))
    return out


@functools.lru_cache(maxsize=None)
def content(amp):
    """shift_noise at one amplitude as content(w, h, n, seed) — one object per amplitude, so that the record caches of test_gpu_cabac_header key on it"""
    return functools.partial(shift_noise, amp=amp)


def ip_records(amp, w, h, n, seed=1, **over):
    return _ip_records(content(amp), w, h, n, seed, tuple(sorted(over.items())))


def b_records(amp, w, h, types, seed=1, **over):
    return _b_records(content(amp), w, h, types, seed, tuple(sorted(over.items())))


def ip_run_any(gpu, w, h, frames, **over):
    """ip_run, also for sessions that carry no context variables (no RD, or CAVLC): there records, levels and reconstruction"""
    kw = dict(IP, **over)
    if kw["rd"] and kw["cabac"]:
        return ip_run(gpu, w, h, frames, **over)
    from gpu_enc import GpuEncoder
    cfg = O.default_config(w, h, **kw)
    og, gg = O.OracleEncoder(cfg), GpuEncoder(cfg)
    for i, f in enumerate(frames):
        st = 2 if i == 0 else 0
        o_mb, o_lv = og.encode(f, st)
        g_mb, g_lv = gg.encode([f], st)
        compare(f"{w}x{h} {over} frame {i}", (w + 15) // 16, g_mb[0], o_mb, g_lv[0], o_lv, gg.recon(0), og.recon())
    og.close(); gg.close()


def n_i4(mbs):
    return int((mbs["type"] == MB_I4x4).sum())


def i4_modes(mbs):
    return set(mbs["i4_mode"][mbs["type"] == MB_I4x4].ravel().tolist())


# ---- 1. I pictures: interior, top row, left column, a last column whose block 5 has no top-right ----
@pytest.mark.parametrize("amp", [2, 8, 20])
@pytest.mark.parametrize("w,h", [(64, 48), (96, 64)])
def test_i_picture_nine_modes(gpu, w, h, amp):
    mbs = ip_records(amp, w, h, 1)[0][0]
    print(n_i4(mbs), "Intra_4x4 of", len(mbs), sorted(i4_modes(mbs)))
    assert n_i4(mbs) >= 5 and len(i4_modes(mbs)) == 9
    ip_run(gpu, w, h, shift_noise(w, h, 1, 1, amp))


# ---- 2. no neighbours, left only, top only: the short mode lists ----
@pytest.mark.parametrize("w,h", [(16, 16), (32, 16), (16, 32)])
def test_i_picture_short_mode_lists(gpu, w, h):
    mbs = ip_records(20, w, h, 1)[0][0]
    assert n_i4(mbs) == len(mbs), mbs["type"]
    ip_run(gpu, w, h, shift_noise(w, h, 1, 1, 20))


# ---- 3. P pictures: the exit threshold swept by the noise ----
@pytest.mark.parametrize("amp,least", [(2, 0), (8, 2), (20, 4)])
def test_p_pictures_exit_threshold_sweep(gpu, amp, least):
    w, h = 96, 64
    cnt = [n_i4(mbs) for mbs, lv in ip_records(amp, w, h, 3)[1:]]
    print("Intra_4x4 macroblocks of the P pictures:", cnt)
    assert all(c == 0 for c in cnt) if least == 0 else all(c >= least for c in cnt), cnt
    ip_run(gpu, w, h, shift_noise(w, h, 3, 1, amp))


# ---- 4. B pictures (the b_type_cost term) ----
@pytest.mark.parametrize("amp", [8, 20])
def test_b_pictures_exit_threshold_sweep(gpu, amp):
    w, h, types = 96, 64, "IBBBPBBBP"
    cnt = [n_i4(mbs) for pt, mbs, lv in b_records(amp, w, h, types) if pt >= 3]
    print("Intra_4x4 macroblocks of the B pictures:", cnt)
    assert len(cnt) == 6 and (all(c >= 3 for c in cnt) if amp == 20 else all(c <= 1 for c in cnt)), cnt
    run(gpu, w, h, types, 1, frames=shift_noise(w, h, len(types), 1, amp))


# ---- 5. the other routes through the same loop: one I and one P picture, and a B mini-GOP where the instantiation has B slices ----
NO_RD = dict(rd=0, trellis=0, psy=0, psy_rd_q8=0)
ROUTES = {
    "rd_off_subme5": dict(NO_RD, subme=5),                               # no slack on the threshold, favoured-direction mode lists
    "subme2_sad": dict(NO_RD, subme=2),                                  # SAD instead of SATD
    "trellis2": dict(trellis=127),                                       # the search in the analysis' block encodes: both blocks of a round in one call
    "trellis2_psy": dict(trellis=127, psy_trellis_q8=38),                # ... with the source transforms of the two blocks idxB - idxA apart
    "subme8": dict(subme=8, rd=63),                                      # every mode; the refinement's inputs
    "subme9": dict(subme=9, rd=63),
    "cavlc": dict(cabac=0, trellis=0),
    "no_8x8dct": dict(dct8x8=0, partitions=3),
    "aq_mode_1": dict(aq_mode=1),                                        # a quantiser per macroblock
}


@pytest.mark.parametrize("name", list(ROUTES))
def test_other_routes(gpu, name):
    over = ROUTES[name]
    w, h = 96, 64          # (at 64x48 the sessions without RD have no Intra_4x4 macroblock in the P picture)
    cnt = [n_i4(mbs) for mbs, lv in ip_records(20, w, h, 2, **over)]
    print("Intra_4x4 macroblocks of I, P:", cnt)
    assert cnt[0] >= 5 and cnt[1] >= 1, cnt
    ip_run_any(gpu, w, h, shift_noise(w, h, 2, 1, 20), **over)
    bcnt = [n_i4(mbs) for pt, mbs, lv in b_records(20, w, h, "IBBP", **over) if pt >= 3]          # every route has B-slice instantiations
    print("... of the B pictures:", bcnt)
    assert sum(bcnt) >= 1, bcnt
    run(gpu, w, h, "IBBP", 1, frames=shift_noise(w, h, 4, 1, 20), **over)


def test_partitions_without_i4x4(gpu):
    """the loop must not run: no Intra_4x4 macroblock where the same content has them with i4x4 allowed"""
    w, h = 64, 48
    assert n_i4(ip_records(20, w, h, 2)[0][0]) >= 5
    assert [n_i4(mbs) for mbs, lv in ip_records(20, w, h, 2, partitions=5)] == [0, 0]
    ip_run(gpu, w, h, shift_noise(w, h, 2, 1, 20), partitions=5)
    assert sum(n_i4(mbs) for pt, mbs, lv in b_records(20, w, h, "IBBP", partitions=5)) == 0
    run(gpu, w, h, "IBBP", 1, frames=shift_noise(w, h, 4, 1, 20), partitions=5)


def test_three_slices(gpu):
    """rows with nothing above them inside the picture"""
    w, h = 96, 192
    mbw = w // 16
    recs = ip_records(20, w, h, 2, slices=3)
    first_rows = [r * mbw + x for r in (4, 8) for x in range(mbw)]          # the first macroblock rows of the second and third slice
    assert sum(int(recs[0][0]["type"][i] == MB_I4x4) for i in first_rows) >= 2 and n_i4(recs[1][0]) >= 1
    ip_run(gpu, w, h, shift_noise(w, h, 2, 1, 20), slices=3)
    run(gpu, w, h, "IBBP", 1, frames=shift_noise(w, h, 4, 1, 20), slices=3)


def test_three_streams(gpu):
    """three streams in lock-step on seeds 2, 3, 4: every stream equals its own checker"""
    from gpu_enc import GpuEncoder
    w, h, seeds = 64, 48, (2, 3, 4)
    for s in seeds:
        cnt = [n_i4(mbs) for mbs, lv in ip_records(20, w, h, 2, seed=s)]
        assert cnt[0] >= 5 and cnt[1] >= 1, (s, cnt)
    seqs = [shift_noise(w, h, 2, s, 20) for s in seeds]
    ogs = [O.OracleEncoder(O.default_config(w, h, **IP)) for _ in seeds]
    gg = GpuEncoder(O.default_config(w, h, streams=len(seeds), **IP))
    for i in range(2):
        st = 2 if i == 0 else 0
        g_mb, g_lv = gg.encode([q[i] for q in seqs], st)
        for s, og in enumerate(ogs):
            o_mb, o_lv = og.encode(seqs[s][i], st)
            compare(f"stream {s} frame {i}", (w + 15) // 16, g_mb[s], o_mb, g_lv[s], o_lv, gg.recon(s), og.recon())
            used = CABAC_CTX_I if st == 2 else CABAC_CTX_P
            np.testing.assert_array_equal(gg.cabac_states(s, 0)[used], og.cabac_states()[used], err_msg=f"context variables of stream {s} after picture {i}")
    for og in ogs:
        og.close()
    gg.close()


def test_noise_reduction_instantiations(gpu):
    """--nr: the denoising instantiations use L.lv4 and the tile as scratch once an inter macroblock is committed.  With zero offsets they code what the
    plain kernels code, so the checker is the reference here too"""
    from test_gpu_nr import Session
    w, h, types = 64, 48, "IPBBP"
    frames = shift_noise(w, h, len(types), 1, 20)
    s = Session(gpu, w, h)
    pics = s.code([frames, frames], types)
    assert not s.offsets().any()
    s.close()
    og = O.OracleEncoder(O.default_config(w, h, **MEDIUM))
    total = 0
    for k, p in enumerate(pics):
        o_mb, o_lv = og.encode_pic(frames[p["disp"]], p["pic"])
        total += n_i4(o_mb) if p["pt"] >= 2 else 0
        for st in range(2):
            compare(f"picture {k} stream {st}", (w + 15) // 16, p["mb"][st], o_mb, p["lv"][st], o_lv, p["recon"][st], og.recon())
    og.close()
    assert total >= 2, "Intra_4x4 macroblocks in the P and B pictures"


# ---- 6. random (seed, amplitude) pairs: wherever the sums cross the threshold ----
def test_random_amplitudes(gpu):
    rnd = random.Random(264)
    w, h = 48, 32
    seen = set()
    for it in range(30):
        seed, amp = rnd.randint(0, 10 ** 6), rnd.randint(1, 40)
        recs = _ip_records(content(amp), w, h, 2, seed, ())
        seen |= {n_i4(recs[1][0]) > 0}
        ip_run(gpu, w, h, shift_noise(w, h, 2, seed, amp))
    assert seen == {False, True}, "P pictures with and without Intra_4x4 macroblocks"

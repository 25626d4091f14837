"""-m gpu: the load balance of the lock-step batch (csrc/encoder.hip k_balance, k_mb.hip.h `s = k.perm[blockIdx.x]`) on streams that differ.  From 512 streams up
workgroup n codes another stream than n; every throughput figure of the project is measured there.  The primitive against its numpy twin, then four batches
of 515 (once 1027) streams whose content, quantisers, direct modes, offsets and vectors differ per stream (tests/balance_cases.py), each stream against the
checker's session of that stream alone — or, where there is no checker (noise reduction), against an encoder created with X264GPU_NO_BALANCE.  After every
picture x264gpu_encoder_last_perm tells whether it ran permuted: a permutation of the streams in which the cheapest stream (0) has lost workgroup 0.

The streams are compared first, the order after them: a permutation that repeats an entry fails at the stream it left uncoded.
tests/test_balance_cases_cpu.py shows on the checker alone that these batches can fail."""
import os

import numpy as np
import pytest

import balance_cases as BC
import bgop
import oracle_lib as O
from balance_cases import H, MBW, NMB, W

pytestmark = pytest.mark.gpu

MBH = NMB // MBW


# ---- what the tests read off an encoder of S streams ----
def all_recons(gg):
    """[S][w * h * 3 / 2]: every stream's reconstruction of the last picture, one copy"""
    from x264vfw_amd import lib
    t, n = gg.torch, W * H * 3 // 2
    out = t.zeros((gg.S, n), dtype=t.uint8, device="cuda")
    for s in range(gg.S):
        lib.check(lib.x264gpu_encoder_get_recon(gg.h, s, out.data_ptr() + s * n, None), "get_recon")
    t.cuda.synchronize()
    return out.cpu().numpy()


def last_perm(gg):
    """perm[workgroup] = stream of the last picture, None when it ran in identity order"""
    from x264vfw_amd import lib
    p = np.full(gg.S, -1, np.int32)
    n = lib.x264gpu_encoder_last_perm(gg.h, p.ctypes.data)
    assert n in (0, gg.S), f"x264gpu_encoder_last_perm returned {n}"
    assert n or (p == -1).all(), "identity order: the array is left alone"
    return p if n else None


def check_perm(perm, S, permuted, tag):
    if not permuted:
        assert perm is None, f"{tag}: ran permuted, but is the first picture of its kind (or the balance is off)"
        return
    assert perm is not None, f"{tag}: ran in identity order"
    assert np.array_equal(np.sort(perm), np.arange(S)), f"{tag}: not a permutation of the streams: {np.setdiff1d(np.arange(S), perm)[:8]} missing"
    assert perm[0] != 0, f"{tag}: the flat stream 0 kept workgroup 0"


def compare_stream(tag, g_mb, g_lv, g_rec, o):
    from test_gpu_pipeline import compare
    compare(tag, MBW, g_mb, o["mb"], g_lv, o["lv"], g_rec, o["recon"])
    assert g_mb.tobytes() == o["mb"].tobytes(), f"{tag}: records differ outside the named fields"


# ---- the primitive ----
@pytest.mark.parametrize("S", BC.PERM_COUNTS)
def test_balance_perm_equals_twin(gpu, S):
    import torch
    for name, t in BC.wtime_arrays(S).items():
        d_t = torch.from_numpy(t.view(np.int32).copy()).cuda()
        d_p = torch.full((S + 2,), -7, dtype=torch.int32, device="cuda")          # a guard entry on either side
        gpu.check(gpu.x264gpu_balance_perm(d_t.data_ptr(), S, d_p.data_ptr() + 4, None), "balance_perm")
        torch.cuda.synchronize()
        got = d_p.cpu().numpy()
        assert got[0] == -7 and got[-1] == -7, f"{name}: wrote outside perm[0 .. S)"
        np.testing.assert_array_equal(got[1:-1], BC.perm_ref(t), err_msg=f"{S} streams, {name}")
        assert np.array_equal(d_t.cpu().numpy().view(np.uint32), t), "the times are read only"


def test_balance_perm_refuses_counts_out_of_range(gpu):
    import torch
    d_t, d_p = torch.zeros(8193, dtype=torch.int32, device="cuda"), torch.full((8193,), -7, dtype=torch.int32, device="cuda")
    for S in (0, -1, 8193):
        assert gpu.x264gpu_balance_perm(d_t.data_ptr(), S, d_p.data_ptr(), None) == -1, S          # X264GPU_EINVAL
    assert gpu.x264gpu_balance_perm(None, 4, d_p.data_ptr(), None) == -1 and gpu.x264gpu_balance_perm(d_t.data_ptr(), 4, None, None) == -1
    torch.cuda.synchronize()
    assert (d_p.cpu().numpy() == -7).all()


# ---- I / P pictures ----
def test_ip_pictures_permuted_streams_equal_the_checker(gpu):
    """x264gpu_encode_frames, I P P I P P with AQ mode 1 (k_aq writes mbqp per stream, the loop reads it through the permuted index): every stream against the
    checker's session of its sequence"""
    from gpu_enc import GpuEncoder
    S = BC.S_DEFAULT
    gg = GpuEncoder(O.default_config(W, H, streams=S, **BC.IP_KW))
    seq = [BC.seq_of(s, S) for s in range(S)]
    for i, st in enumerate(BC.IP_TYPES):
        g_mb, g_lv = gg.encode(BC.batch_frames(S, len(BC.IP_TYPES), i), st)
        perm, rec = last_perm(gg), all_recons(gg)
        for s in range(S):
            compare_stream(f"I/P picture {i} stream {s} ({BC.seq_name(seq[s])})", g_mb[s], g_lv[s], rec[s], BC.ip_session(seq[s])[i])
        check_perm(perm, S, i in BC.IP_PERMUTED, f"I/P picture {i}")
    gg.close()


# ---- B pictures, the headline toolset ----
@pytest.mark.parametrize("S", [BC.S_DEFAULT, BC.S_BIG])
def test_b_pictures_permuted_streams_equal_the_checker(gpu, S):
    """x264gpu_encode_pictures over IBBBPBBBPBBBP with --weightp 2 and the pyramid: per stream its own quantiser, on every second picture a float quantiser
    under AQ, its own direct mode with the probe counts of --direct auto.  Records, levels, reconstruction and probe counts of every stream, the context
    variables of four of them, and stream 1's pictures through the host writer and the checker's decoder"""
    from gpu_enc import GpuEncoder
    from test_gpu_bframes import USED_CTX
    from x264vfw_amd import lib
    kw = BC.b_kw()
    cfg = O.default_config(W, H, **kw)
    gg = GpuEncoder(O.default_config(W, H, streams=S, **kw))
    dpb, order = BC.b_plan()
    n, keys = len(BC.B_TYPES), BC.b_keys(S)
    permuted = BC.permuted_pictures([pt for _, pt in order])
    assert len(permuted) == len(order) - 4
    stream = dpb.headers(W, H, BC.base_qp(2), cfg.chroma_qp_offset, kw["refs"], cfg.dct8x8, cfg.weightb)
    recons1 = []
    for i, (disp, pt) in enumerate(order):
        pic, _ = dpb.plan(pt, disp, bgop.follow_of(order, i))
        if pt >= 3:
            dpb.set_direct(pic, 1, 1)          # stream 1's mode, for the slice headers of the stream written below
        pics = [BC.stream_pic(pic, i, pt, *BC.stream_controls(s)) for s in range(S)]
        g_mb, g_lv = gg.encode_pics(BC.batch_frames(S, n, disp), pics)
        perm, rec = last_perm(gg), all_recons(gg)
        scores = np.zeros((S, 2), np.int32)
        if pt >= 3:
            lib.check(lib.x264gpu_encoder_direct_scores(gg.h, scores.ctypes.data), "direct_scores")
        for s in range(S):
            o = BC.b_session(*keys[s])[i]
            tag = f"picture {i} (display {disp}, type {pt}) stream {s} ({BC.seq_name(keys[s][0])}, controls {keys[s][1:]})"
            compare_stream(tag, g_mb[s], g_lv[s], rec[s], o)
            assert pt < 3 or tuple(int(v) for v in scores[s]) == o["dscore"], f"{tag}: skip-probe counts {scores[s]} vs {o['dscore']}"
        for s in (0, 1, S // 2, S - 1):
            assert pt <= 1 or np.array_equal(gg.cabac_states(s, 0)[USED_CTX], BC.b_session(*keys[s])[i]["states"][USED_CTX]), f"picture {i} stream {s}: CABAC context variables differ"
        check_perm(perm, S, i in permuted, f"picture {i} (type {pt})")
        stream += dpb.slice(MBW, MBH, pics[1].qp, BC.base_qp(2), 0, 0 if cfg.deblock else 1, kw["refs"], cfg.dct8x8, g_mb[1], g_lv[1])
        recons1.append(rec[1])
        dpb.commit()
    dec = O.h264_decode(stream, len(order), W, H)
    assert len(dec) == len(order)
    for i, (d, r) in enumerate(zip(dec, recons1)):
        assert np.array_equal(d, r), f"picture {i} of stream 1's bitstream decodes differently"
    gg.close(); dpb.close()


# ---- side rows ----
def test_side_rows_follow_their_streams(gpu):
    """x264gpu_encoder_set_mb_qp_offsets ([S][nmb] floats) and x264gpu_encoder_set_lowres_mvs ([S][nmb][2]), distinct per stream, I P P: every stream
    against the checker fed that stream's rows (as test_external_mb_qp_offsets and test_lookahead_vectors_enter_the_16x16_candidates feed one)"""
    import torch
    from gpu_enc import GpuEncoder
    from x264vfw_amd import lib
    S = BC.S_DEFAULT
    off, mv = BC.side_rows(S)
    gg = GpuEncoder(O.default_config(W, H, streams=S, **BC.SIDE_KW))
    d_off, d_mv = torch.from_numpy(off.copy()).cuda(), torch.from_numpy(mv.copy()).cuda()
    lib.check(lib.x264gpu_encoder_set_mb_qp_offsets(gg.h, d_off.data_ptr()), "set_mb_qp_offsets")
    lib.check(lib.x264gpu_encoder_set_lowres_mvs(gg.h, d_mv.data_ptr()), "set_lowres_mvs")
    for i, st in enumerate(BC.SIDE_TYPES):
        g_mb, g_lv = gg.encode(BC.batch_frames(S, len(BC.SIDE_TYPES), i), st)
        perm, rec = last_perm(gg), all_recons(gg)
        for s in range(S):
            compare_stream(f"side rows picture {i} stream {s} ({BC.seq_name(BC.seq_of(s, S))})", g_mb[s], g_lv[s], rec[s], BC.side_session(s, S)[i])
        check_perm(perm, S, i == 2, f"side rows picture {i}")
    gg.close()


# ---- noise reduction ----
def _nr_run(lib, S):
    """the NR case on a fresh encoder: per coded picture dict(pt, mb, lv, recon, sums, perm), and the offsets the streams ended with"""
    import torch
    from gpu_enc import GpuEncoder
    import host_lib as HL
    kw = BC.nr_kw()
    gg = GpuEncoder(O.default_config(W, H, streams=S, **kw))
    dpb, order = bgop.HostDpb(HL, kw["refs"], 3, 1, weightp=0), bgop.schedule(BC.NR_TYPES, 1)
    d_off = torch.zeros((S, 192), dtype=torch.int16, device="cuda")
    d_pic = torch.full((S, 1552), 0xCD, dtype=torch.uint8, device="cuda")
    # x264gpu_nr_update takes one strength a call: the three strengths each keep offsets and a state for all streams, stream s takes those of its own
    grown = [(torch.zeros_like(d_off), torch.zeros((S, 1552), dtype=torch.uint8, device="cuda")) for _ in BC.NR_STRENGTHS]
    lib.check(lib.x264gpu_encoder_set_nr(gg.h, d_off.data_ptr(), d_pic.data_ptr()), "set_nr")
    out = []
    for i, (disp, pt) in enumerate(order):
        pic, _ = dpb.plan(pt, disp, bgop.follow_of(order, i))
        pic.qp = bgop.pic_qp(pt, *BC.NR_QPS)
        mb, lv = gg.encode_pics(BC.batch_frames(S, len(BC.NR_TYPES), disp), [pic] * S)
        out.append(dict(pt=pt, mb=mb, lv=lv, perm=last_perm(gg), recon=all_recons(gg), sums=d_pic.cpu().numpy()[:, :1548].copy()))
        for j, strength in enumerate(BC.NR_STRENGTHS):
            lib.check(lib.x264gpu_nr_update(grown[j][0].data_ptr(), grown[j][1].data_ptr(), d_pic.data_ptr(), S, strength, None), "nr_update")
            d_off[j::3] = grown[j][0][j::3]
        torch.cuda.synchronize()
        dpb.commit()
    off = d_off.cpu().numpy().view(np.uint16).reshape(S, 3, 64)
    gg.close(); dpb.close()
    return out, off


def test_noise_reduction_rows_follow_their_streams(gpu):
    """the denoising instantiations read nr_off[stream] and write nr_part[stream]: offsets grown per stream from strengths 0 / 100 / 1000, the balanced encoder
    against one created with X264GPU_NO_BALANCE (the library reads it at create) — and the strength-0 streams against the checker, whose plain session they code"""
    S = BC.S_DEFAULT
    old = os.environ.pop("X264GPU_NO_BALANCE", None)
    try:
        bal, off_b = _nr_run(gpu, S)
        os.environ["X264GPU_NO_BALANCE"] = "1"
        ident, off_i = _nr_run(gpu, S)
    finally:
        os.environ.pop("X264GPU_NO_BALANCE", None)
        if old is not None:
            os.environ["X264GPU_NO_BALANCE"] = old
    assert not off_i[0::3].any() and off_i[1::3].any(axis=(1, 2)).sum() > S // 4 and (off_i[2::3].astype(np.int64).sum() > off_i[1::3].astype(np.int64).sum())
    permuted = BC.permuted_pictures([p["pt"] for p in bal])
    assert len(permuted) == 4
    for i, (a, b) in enumerate(zip(bal, ident)):
        for s in range(S):
            tag = f"NR picture {i} (type {a['pt']}) stream {s} ({BC.seq_name(BC.seq_of(s, S))}, strength {BC.NR_STRENGTHS[s % 3]})"
            compare_stream(tag + " balanced vs identity order", a["mb"][s], a["lv"][s], a["recon"][s], dict(mb=b["mb"][s], lv=b["lv"][s], recon=b["recon"][s]))
            assert np.array_equal(a["sums"][s], b["sums"][s]), f"{tag}: statistics differ"
            if s % 3 == 0:
                compare_stream(tag + " vs the checker's plain session", b["mb"][s], b["lv"][s], b["recon"][s], BC.nr_plain_session(BC.seq_of(s, S))[i])
        assert a["pt"] <= 1 or a["sums"].any(axis=1).sum() > S // 2, f"NR picture {i}: no statistics"
        check_perm(a["perm"], S, i in permuted, f"NR picture {i} (type {a['pt']})")
        check_perm(b["perm"], S, False, f"NR picture {i} without the balance")
    np.testing.assert_array_equal(off_b, off_i)
    # the offsets matter: a stream of strength 1000 codes other levels than the checker's plain session of its sequence
    moved = sum(any(ident[i]["lv"][s].tobytes() != BC.nr_plain_session(BC.seq_of(s, S))[i]["lv"].tobytes() for i in range(len(ident))) for s in range(2, S, 3))
    assert moved > S // 6, moved

"""-m gpu: the device pipeline against the CPU checker on full-range and saturated pictures (tests/hard_content.py): samples over all of 0..255, pictures
of 0 and 255 alone, flat pictures at both rails.  The comparisons are the suite's own (records byte for byte, levels, reconstruction, CABAC context
variables, the device's B streams through the checker decoder); what is new is the content: levels beyond 2047 (the long CAVLC escape, the CABAC
Exp-Golomb suffix, trellis and decimation on them), the reconstruction clip at 0 and 255, intra prediction from rail-valued neighbours, the packed
16-bit Hadamard sums at their largest inputs, flat and all-255 macroblocks in both AQ implementations, costs of 10^7 in the search keys.
tests/test_hard_content_cpu.py asserts on the checker alone that every case below reaches what it is there for, and that the checker's own B streams
decode to its reconstruction."""
import numpy as np
import pytest

import hard_content as HC
import oracle_lib as O
from test_gpu_bframes import run as run_b
from test_gpu_lookahead import ADAPT, mbtree_walk_case, run_case, run_slicetype
from test_gpu_pipeline import CABAC_CTX_I, CABAC_CTX_P, compare

pytestmark = pytest.mark.gpu


# ---- a. I / P pictures ----
@pytest.mark.parametrize("case", HC.IP_CASES, ids=[c["id"] for c in HC.IP_CASES])
def test_ip_pipeline_bitexact(gpu, case):
    from gpu_enc import GpuEncoder
    w, h, kw = case["w"], case["h"], case["kw"]
    cfg = O.default_config(w, h, **kw)
    og, gg = O.OracleEncoder(cfg), GpuEncoder(cfg)
    ctx = kw.get("cabac") and kw.get("rd")
    for i, f in enumerate(HC.frames_of(case)):
        st = HC.ip_slice_type(i)
        o_mb, o_lv = og.encode(f, st)
        g_mb, g_lv = gg.encode([f], st)
        compare(f"{case['id']} frame {i}", (w + 15) // 16, g_mb[0], o_mb, g_lv[0], o_lv, gg.recon(0), og.recon())
        if ctx:
            used = CABAC_CTX_I if st == 2 else CABAC_CTX_P
            np.testing.assert_array_equal(gg.cabac_states(0, kw.get("slices", 1) - 1)[used], og.cabac_states()[used], err_msg=f"context variables after picture {i}")
    og.close(); gg.close()


def test_ip_multistream_one_kind_each(gpu):
    """four lock-step streams, each with another kind of content, each equal to its own checker (context variables included)"""
    from gpu_enc import GpuEncoder
    m = HC.MULTI
    w, h, S = m["w"], m["h"], len(m["kinds"])
    seqs = [HC.KINDS[k](w, h, m["n"], m["seed"] + s) for s, k in enumerate(m["kinds"])]
    gg = GpuEncoder(O.default_config(w, h, streams=S, **m["kw"]))
    ogs = [O.OracleEncoder(O.default_config(w, h, **m["kw"])) for _ in range(S)]
    for i in range(m["n"]):
        st = HC.ip_slice_type(i)
        g_mb, g_lv = gg.encode([seqs[s][i] for s in range(S)], st)
        for s in range(S):
            o_mb, o_lv = ogs[s].encode(seqs[s][i], st)
            compare(f"stream {s} ({m['kinds'][s]}) frame {i}", (w + 15) // 16, g_mb[s], o_mb, g_lv[s], o_lv, gg.recon(s), ogs[s].recon())
            used = CABAC_CTX_I if st == 2 else CABAC_CTX_P
            np.testing.assert_array_equal(gg.cabac_states(s, 0)[used], ogs[s].cabac_states()[used], err_msg=f"stream {s} picture {i}")
    for o in ogs:
        o.close()
    gg.close()


# ---- b. B pictures ----
@pytest.mark.parametrize("case", HC.B_CASES, ids=[c["id"] for c in HC.B_CASES])
def test_b_pictures_bitexact_and_decodable(gpu, case):
    run_b(gpu, case["w"], case["h"], case["types"], case["seed"], pyramid=case["pyramid"], weightp=case["weightp"], weights=case["weights"],
          frames=HC.frames_of(case), direct=case["direct"], qps=case["qps"], **case["over"])


# ---- c. lookahead ----
@pytest.mark.parametrize("w,h", HC.LA_SIZES)
@pytest.mark.parametrize("kind", list(HC.KINDS))
def test_lookahead_cost_bitexact(gpu, kind, w, h):
    run_case(w, h, HC.KINDS[kind](w, h, HC.LA_FRAMES, 30))


def test_lookahead_flash_with_a_reset(gpu):
    run_case(80, 48, HC.flash(80, 48, 6, 0), resets=(3,))


@pytest.mark.parametrize("kind", list(HC.KINDS))
def test_aq_offsets_all_modes_bitexact(gpu, kind):
    """x264gpu_lookahead_aq_offsets (mode 1) and _aq_offsets_mode 2 / 3 against the checker, byte for byte: flat macroblocks (energy 0) and all-255
    ones (sum x sum within 0.8 % of 2^32) among them"""
    from gpu_enc import GpuLookahead
    w, h = 80, 48
    frames = HC.KINDS[kind](w, h, 2, 31)
    gl = GpuLookahead(w, h, streams=2)
    for strength in (O.AQ1, float(np.float32(1.55955))):
        g = gl.aq_offsets(frames, strength).cpu().numpy()
        for s in range(2):
            assert g[s].tobytes() == O.aq_offsets(frames[s], w, h, strength).tobytes(), f"mode 1 strength {strength} picture {s}"
    for mode in (2, 3):
        g = gl.aq_offsets_mode(frames, mode, 1.0).cpu().numpy()
        for s in range(2):
            o = O.aq_offsets_mode(frames[s], w, h, mode, 1.0)
            assert g[s].tobytes() == o.tobytes(), f"mode {mode} picture {s}: {np.nonzero(g[s] != o)[0][:5]}"
    gl.close()


@pytest.mark.parametrize("kind", HC.SLICETYPE_KINDS)
def test_slicetype_costs_bitexact(gpu, kind):
    run_slicetype(HC.LA_W, HC.LA_H, 5, 0, ADAPT[:12], frames=HC.KINDS[kind](HC.LA_W, HC.LA_H, 5, 32), do_edges=1)


@pytest.mark.parametrize("kind,types,seed", HC.MBTREE_CASES, ids=[f"{k}-{len(t)}" for k, t, _ in HC.MBTREE_CASES])
def test_mbtree_through_b_pictures_bitexact(gpu, kind, types, seed):
    """the last case runs the propagate cost into its saturation at 32767 (asserted on the checker in tests/test_hard_content_cpu.py)"""
    mbtree_walk_case(HC.LA_W, HC.LA_H, types, True, False, True, 0, frames=HC.KINDS[kind](HC.LA_W, HC.LA_H, len(types), seed))

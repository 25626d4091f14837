"""CPU: what the checker makes of the full-range and saturated pictures of tests/hard_content.py, for every (content, configuration) pair that
tests/test_gpu_hard_content.py compares the device with — the content must reach what it is there for (levels beyond 2047, reconstruction at
the rails, flat macroblocks, every family of B macroblock types in every B case, costs beyond 2^20), and for every B case the checker's own stream (host CABAC /
CAVLC writer) must decode, in the checker decoder, to the checker's reconstruction: that is what tells a checker error from a device error."""
import functools

import numpy as np
import pytest

import bgop
import hard_content as HC
import host_lib as HL
import oracle_lib as O
from test_gpu_bframes import MEDIUM          # the toolset test_gpu_bframes.run gives the device: one dict for both files

IP = {c["id"]: c for c in HC.IP_CASES}
B = {c["id"]: c for c in HC.B_CASES}


@functools.lru_cache(maxsize=None)
def ip_stats(cid):
    """(largest |level|, share of reconstructed samples at 0 / 255, largest record cost) of an I / P case on the checker"""
    c = IP[cid]
    og = O.OracleEncoder(O.default_config(c["w"], c["h"], **c["kw"]))
    lv_max = cost_max = 0
    recons = []
    for i, f in enumerate(HC.frames_of(c)):
        mbs, lv = og.encode(f, HC.ip_slice_type(i))
        lv_max = max(lv_max, int(np.abs(lv.astype(np.int32)).max()))
        cost_max = max(cost_max, int(mbs["cost"].max()))
        recons.append(og.recon())
    og.close()
    return lv_max, HC.rail_share(recons), cost_max


@functools.lru_cache(maxsize=None)
def b_run(cid):
    """a B case through the checker and the host writer: (stream, reconstructions, coding order, [(picture type, records, levels)])"""
    c = B[cid]
    kw = dict(MEDIUM, **c["over"])
    cfg = O.default_config(c["w"], c["h"], **kw)

    class Keep(O.OracleEncoder):
        def encode_pic(self, f, pic):
            mbs, lv = super().encode_pic(f, pic)
            self.kept.append((pic.slice_type, mbs.copy(), lv.copy()))
            return mbs, lv
    enc = Keep(cfg)
    enc.kept = []
    qi, qp, qb = c["qps"]
    stream, recons, order, _ = bgop.encode_gop(HL, enc, HC.frames_of(c), c["types"], cfg, qi, qp, qb, kw["refs"], 3, c["pyramid"], c["weightp"], None, c["weights"], c["direct"])
    enc.close()
    return stream, recons, order, [(pt, m, lv) for (disp, pt), (_, m, lv) in zip(order, enc.kept)]


@pytest.mark.parametrize("cid", list(IP))
def test_ip_content_reaches_its_target(cid):
    c = IP[cid]
    lv_max, rails, cost_max = ip_stats(cid)
    print(f"{cid}: largest level {lv_max}, rail share {rails:.3f}, largest cost {cost_max}")
    if c["big_levels"]:
        assert lv_max > 2047, lv_max
    if c["kind"] in HC.BINARY and max(c["kw"]["qp_i"], c["kw"]["qp_p"]) <= HC.MID_QP:
        assert rails >= 0.25, rails
    if c["big_cost"]:
        assert cost_max > 1 << 20, cost_max


def b_stats(cid):
    """(bi-predicted inter, direct / skip, intra macroblocks of the B pictures; largest |level|; rail share; largest cost of a record that holds one)"""
    _, recons, _, kept = b_run(cid)
    bi = direct = intra = lv_max = cost_max = 0
    for pt, m, lv in kept:
        lv_max = max(lv_max, int(np.abs(lv.astype(np.int32)).max()))
        ty = m["type"]
        cost_max = max(cost_max, int(m["cost"][(ty <= 6) if pt < 3 else (ty <= 2)].max(initial=0)))          # (B inter records keep list 1's vectors in these bytes)
        if pt >= 3:
            inter = (ty == O.MB_B_INTER) | (ty == O.MB_B_8x8)
            bi += int((inter & ((m["ref"] >= 0) & (O.mb_ref1(m) >= 0)).any(axis=1)).sum())
            direct += int(((ty == O.MB_B_DIRECT) | (ty == O.MB_B_SKIP)).sum())
            intra += int((ty <= 2).sum())
    return bi, direct, intra, lv_max, HC.rail_share(recons), cost_max


@pytest.mark.parametrize("cid", list(B))
def test_b_case_decodes_and_reaches_its_target(cid):
    c = B[cid]
    stream, recons, order, _ = b_run(cid)
    dec = O.h264_decode(stream, len(order), c["w"], c["h"])
    assert len(dec) == len(order)
    for k, (d, r) in enumerate(zip(dec, recons)):
        assert np.array_equal(d, r), f"picture {k} (display {order[k][0]}, type {order[k][1]}) of the checker's stream decodes differently"
    bi, direct, intra, lv_max, rails, cost_max = b_stats(cid)
    print(f"{cid}: bi {bi}, direct / skip {direct}, intra {intra}, largest level {lv_max}, rail share {rails:.3f}, largest cost {cost_max}")
    assert bi >= 1 and direct >= 1 and intra >= 1, (bi, direct, intra)          # every family of B macroblock types in every case
    if c["big_levels"]:
        assert lv_max > 2047, lv_max
    if c["kind"] in HC.BINARY and max(c["qps"]) <= HC.MID_QP:
        assert rails >= 0.25, rails
    if c["big_cost"]:
        assert cost_max > 1 << 20, cost_max


@pytest.mark.parametrize("kind,types,seed", HC.MBTREE_CASES, ids=[f"{k}-{len(t)}" for k, t, _ in HC.MBTREE_CASES])
def test_mbtree_walk_on_the_checker(kind, types, seed):
    """the macroblock-tree cases of the device test on the checker alone: the tree moves quantisers, and the long static case drives the
    propagate cost into its saturation at 32767"""
    from mbtree_walk import macroblock_tree
    w, h, n = HC.LA_W, HC.LA_H, len(types)
    frames = HC.KINDS[kind](w, h, n, seed)
    og = O.OracleSlicetype(w, h, slots=n + 1, do_edges=1)
    for i, f in enumerate(frames):
        og.put(i, f); og.set_aq(i, O.aq_offsets(f, w, h))
    oo = macroblock_tree(og, list(range(n)), types, n - 1, False, True, O.TREE)
    assert oo and all((oo[k] != O.aq_offsets(frames[k], w, h)).any() for k in oo)
    top = max(int(og.propagate_cost(i).max()) for i in range(n))
    print(f"{kind} x {n}: largest propagate cost {top}")
    assert top == 32767 or n < 40, top
    og.close()


def test_flash_pictures_are_flat():
    """every macroblock of every flash picture has zero variance, luma and chroma, at every size the cases use"""
    for w, h in set(HC.SIZES) | set(HC.LA_SIZES):
        for f in HC.flash(w, h, 6, 1)[1:]:
            assert all(len(np.unique(p)) == 1 for p in (f[:w * h], f[w * h:w * h * 5 // 4], f[w * h * 5 // 4:]))


def test_flash_b_cases_are_flat_outside_the_patches():
    """the B cases lay three patches over the kind's pictures (HC.b_patches); every other macroblock of the flash cases stays flat"""
    for c in HC.B_CASES:
        if c["kind"] != "flash":
            continue
        w, h = c["w"], c["h"]
        for f in HC.frames_of(c)[1:]:
            y = f[:w * h].reshape(h, w)
            for my in range(0, h, 16):
                for mx in range(0, w, 16):
                    if (mx // 16, my // 16) not in HC.B_PATCH_MBS:
                        assert len(np.unique(y[my:my + 16, mx:mx + 16])) == 1, (c["id"], mx, my)


def test_slow_toolset_runs_at_every_quantiser_triple():
    """slow's toolset (umh, trellis 2, subme 9, RD refinement) meets every quantiser triple, and at (0, 1, 2) a case designated for levels beyond 2047"""
    slow = [c for c in HC.B_CASES if c["over"] == HC.SLOW_B]
    assert {c["qps"] for c in slow} == set(HC.B_QPS)
    assert any(c["big_levels"] for c in slow if c["qps"] == HC.B_QPS[0])
    assert any(c["big_cost"] for c in slow if c["qps"] == HC.B_QPS[2])


def test_generators_are_deterministic_and_full_range():
    for name, g in HC.KINDS.items():
        a, b = g(70, 38, 3, 4), g(70, 38, 3, 4)
        assert all(x.dtype == np.uint8 and x.shape == (70 * 38 * 3 // 2,) and np.array_equal(x, y) for x, y in zip(a, b)), name
        allf = np.concatenate(g(64, 48, 4, 4))
        assert allf.min() == 0 and allf.max() == 255, name
        if name in HC.BINARY:
            assert set(np.unique(allf).tolist()) == {0, 255}, name

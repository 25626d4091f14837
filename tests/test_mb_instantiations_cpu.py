"""CPU: the table of the macroblock loop's instantiations (tests/mb_instantiations.py) against the sources, and its rows on the checker alone.

Completeness: the launch sites of x264vfw_amd/csrc/mb_slice_*.hip, template defaults filled in, are exactly the ids the table claims — an instantiation added
without a row fails here, before anything runs on a device.  Not vacuous: on the checker every row's pictures hold what makes its kernels do work — coded luma in
every slice type the row claims, a searched inter macroblock in P and in B pictures, and under psy-trellis levels that the strength really moves."""
import functools
import glob
import os
import re

import numpy as np
import pytest

import bgop
import host_lib as HL
import mb_instantiations as T
import oracle_lib as O

CSRC = os.path.join(O.ROOT, "x264vfw_amd", "csrc")
SITE = re.compile(r"mb_launch<([^>]*)>\s*\(")
QPS = (20, 23, 25)          # test_gpu_bframes.run's quantisers of I, P and disposable B pictures


def launch_sites(texts):
    """-> ({id: [unit file, ..]}, number of sites) of the mb_launch<M, ME, PS, RD = 0, BS = false, PSY = false, NR = false> calls in {file name: text}"""
    found, n = {}, 0
    val = {"true": 1, "false": 0}
    for name, text in sorted(texts.items()):
        for args in SITE.findall(text):
            a = [val[x] if x in val else int(x) for x in (s.strip() for s in args.split(","))]
            assert 3 <= len(a) <= 7, (name, args)
            a += [0] * (7 - len(a))
            found.setdefault(T.mb_id(*a), []).append(name)
            n += 1
    return found, n


def unit_texts():
    return {os.path.basename(p): open(p).read() for p in glob.glob(os.path.join(CSRC, "mb_slice_*.hip"))}


def test_the_table_names_every_instantiation_and_no_other():
    texts = unit_texts()
    found, sites = launch_sites(texts)
    assert len(texts) == 39 and sites == 103 and len(found) == 103, (len(texts), sites, len(found))
    assert all(len(v) == 1 for v in found.values()), "an instantiation has one launch site"
    missing, extra = sorted(set(found) - T.ALL_IDS), sorted(T.ALL_IDS - set(found))
    assert not missing, f"launched in csrc/ without a row in tests/mb_instantiations.py: {[(T.id_name(i), found[i]) for i in missing]}"
    assert not extra, f"rows claim instantiations that csrc/ does not launch: {[T.id_name(i) for i in extra]}"
    assert len(T.ALL_IDS) == 103
    # the check bites: without one launch site the sets differ
    name = "mb_slice_b_esa.hip"
    cut = dict(texts, **{name: texts[name].replace("mb_launch<2, 3, true, 4, true>(k, streams, st)", "(void)0", 1)})
    assert cut[name] != texts[name]
    assert T.ALL_IDS - set(launch_sites(cut)[0]) == {T.mb_id(2, 3, True, 4, True)}


def test_ids_round_trip_and_rows_are_well_formed():
    for r in T.ROWS:
        assert set(r["ids"]) <= set(r["types"]) and r["types"][0] == "I", r["name"]
        for st, i in r["ids"].items():
            M, ME, PS, RD, BS, PSY, NR = T.id_tuple(i)
            assert T.mb_id(M, ME, PS, RD, BS, PSY, NR) == i
            assert PS == (st != "I") and BS == (st == "B") and NR == r["nr"] and PSY == bool(r["over"].get("psy_trellis_q8")), (r["name"], T.id_name(i))
        assert (r["harness"] == "nr") == r["nr"]


@functools.lru_cache(maxsize=None)
def checker_pictures(name, psy_trellis_q8=None):
    """the row on the checker: [(slice type letter, records, levels)] in coding order; psy_trellis_q8: instead of the row's own strength"""
    r = T.BY_NAME[name]
    kw = T.config_kw(r)
    if psy_trellis_q8 is not None:
        kw["psy_trellis_q8"] = psy_trellis_q8
    cfg = O.default_config(T.W, T.H, **kw)
    frames = T.frames_of(r)
    out = []
    if r["harness"] == "ip":
        og = O.OracleEncoder(cfg)
        for i, f in enumerate(frames):
            mbs, lv = og.encode(f, 2 if i == 0 else 0)
            out.append((r["types"][i], mbs, lv))
        og.close()
        return out

    class Keep(O.OracleEncoder):
        def encode_pic(self, f, pic):
            mbs, lv = super().encode_pic(f, pic)
            out.append(("P" if pic.slice_type == O.SLICE_P else "B" if pic.slice_type == O.SLICE_B else "I", mbs.copy(), lv.copy()))
            return mbs, lv
    enc = Keep(cfg)
    bgop.encode_gop(HL, enc, frames, r["types"], cfg, *QPS, kw["refs"], 3, 1)
    enc.close()
    return out


PLAIN_ROWS = [r["name"] for r in T.ROWS if not r["nr"]]


@pytest.mark.parametrize("name", PLAIN_ROWS)
def test_row_is_not_vacuous_on_the_checker(name):
    r = T.BY_NAME[name]
    pics = checker_pictures(name)
    assert [t for t, _, _ in pics].count("I") == 1 and len(pics) == len(r["types"])
    luma = lambda lv: lv[:, :272]          # luma levels and the Intra_16x16 luma DC (x264gpu.h: the layout of a macroblock's levels)
    for st in r["ids"]:
        of_type = [(m, lv) for t, m, lv in pics if t == st]
        assert of_type, f"no {st} picture"
        coded = sum(int(luma(lv).any(axis=1).sum()) for _, lv in of_type)
        assert coded >= 1, f"{st} pictures: no macroblock with luma levels"
        ty = np.concatenate([m["type"] for m, _ in of_type])
        if st == "P":
            n = int(((ty == O.MB_P_L0) | (ty == O.MB_P_8x8)).sum())
            assert n >= 1, f"P pictures: no inter macroblock that is not a skip ({np.bincount(ty).tolist()})"
        if st == "B":
            n = int(((ty == O.MB_B_INTER) | (ty == O.MB_B_8x8)).sum())          # (more than asked of a row: an intra macroblock would not do)
            assert n >= 1, f"B pictures: no searched inter macroblock, all direct, skipped or intra ({np.bincount(ty).tolist()})"
    moved = {}
    if r["over"].get("psy_trellis_q8"):
        plain = checker_pictures(name, 0)
        for st in r["ids"]:
            moved[st] = sum(not np.array_equal(luma(a[2]), luma(b[2])) for a, b in zip(pics, plain) if a[0] == st)
            assert moved[st] >= 1, f"psy-trellis {r['over']['psy_trellis_q8']} moves no luma level of the {st} pictures"
    print(name, [(t, np.bincount(m["type"], minlength=11).tolist(), int(luma(lv).any(axis=1).sum())) for t, m, lv in pics], moved)

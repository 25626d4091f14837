"""The table of the macroblock loop's instantiations (no GPU import): every k_mb_slice<M, ME, PS, RD, BS, PSY, NR> that x264vfw_amd/csrc/mb_slice_*.hip
launches, and the ROWS that pin them — one small encode each, which reaches up to three of them (its I, P and B kernels).

tests/test_mb_instantiations_cpu.py holds the table against the sources (a launch site without a row fails there) and shows on the checker alone that no
row is vacuous; tests/test_gpu_mb_instantiations.py runs every row on the device, bit for bit against the checker (noise reduction: against the plain
kernel of the same tuple, which this table pins to the checker, and the checker's decoder), and proves through x264gpu_mb_kernels_seen that the row
launched the kernels it names.

An id spells the template tuple in hex digits, as include/x264gpu.h says: M << 12 | ME << 8 | RD << 4 | PS << 3 | BS << 2 | PSY << 1 | NR.
  M   sub-pel neighbourhood margin of the reference cache: 2 samples, 5 from --subme 8 on (B slices: 9)
  ME  0 dia, 1 hex, 2 umh, 3 esa (I slices: 1)
  RD  0 none, 1 CAVLC bit counts, 2 CABAC sizes, 3 + trellis 1, 4 + trellis 2, 5 RD refinement (trellis 0 / 1), 6 refinement + trellis 2,
      7 B slices analysed without RD whose final encode runs the trellis quantiser
  PS  P or B slice; BS B slice; PSY psy-trellis; NR noise reduction"""
from synth import synth_frames

W, H = 64, 48          # 4 x 3 macroblocks: the interior ones have every neighbour
ME_NAMES = ("dia", "hex", "umh", "esa")
PSY_TRELLIS_Q8 = 640          # --psy-rd x:2.5, the largest strength the configuration accepts: the levels move in every slice type of every psy row


def mb_id(M, ME, PS, RD=0, BS=False, PSY=False, NR=False):
    return M << 12 | ME << 8 | RD << 4 | int(PS) << 3 | int(BS) << 2 | int(PSY) << 1 | int(NR)


def id_tuple(i):
    return (i >> 12, i >> 8 & 15, bool(i & 8), i >> 4 & 15, bool(i & 4), bool(i & 2), bool(i & 1))


def id_name(i):
    M, ME, PS, RD, BS, PSY, NR = id_tuple(i)
    t = [str(M), str(ME), "true" if PS else "false", str(RD)] + ["true" if f else "false" for f in (BS, PSY, NR)]
    while len(t) > 3 and t[-1] in ("false", "0"):
        t.pop()
    return f"0x{i:04x} <{', '.join(t)}>"


def _row(name, harness, types, over, I=None, P=None, B=None, seed=1, nr=False):
    return dict(name=name, harness=harness, types=types, over=over, seed=seed, nr=nr, ids={k: v for k, v in (("I", I), ("P", P), ("B", B)) if v is not None})


def _rows():
    """harness "ip": x264gpu_encode_frames over tests/oracle_lib.default_config (test_gpu_pipeline.compare); "b": test_gpu_bframes.run over its MEDIUM
    toolset; "nr": test_gpu_nr.Session over the same toolset.  `over` holds what steers the dispatch (encoder.hip's macroblock-loop launch and the
    launch_mb_slice_* functions): me_method, subme, the rd bits, cabac, trellis, psy_trellis_q8."""
    out = []
    # ---- plain kernels: the six B kernels of every search method, with the I and P kernels the same session launches ----
    nord = dict(rd=0, trellis=0, psy_rd_q8=0, subme=5)
    for m, me in enumerate(ME_NAMES):
        mo = dict(me_method=m, me_range=8) if m == 3 else dict(me_method=m)
        for tag, over, rd_ip, rd_b in (("nord", nord, 0, 0), ("subme6", dict(subme=6), 3, 7), ("cavlc", dict(cabac=0, trellis=0), 1, 1),
                                       ("cabac", dict(trellis=0), 2, 2), ("trellis1", {}, 3, 3), ("trellis2", dict(trellis=127), 4, 4)):
            out.append(_row(f"{me}-{tag}", "b", "IBBP", dict(over, **mo), I=mb_id(2, 1, False, rd_ip), P=mb_id(2, m, True, rd_ip), B=mb_id(2, m, True, rd_b, True),
                            seed=10 + 7 * m + rd_b))
        # --subme 8 / 9 without RD: the P kernel with the 5-sample margin (big_margin in encoder.hip); no B pictures
        out.append(_row(f"{me}-bigmargin", "ip", "IPP", dict(dict(subme=8 + (m & 1), partitions=3, refs=2), **mo), I=mb_id(2, 1, False), P=mb_id(5, m, True), seed=40 + m))
    # ---- --subme 9: RD refinement (hex / umh) ----
    for m in (1, 2):
        for tag, over, rd in (("refine", dict(subme=9, rd=63), 5), ("refine-trellis2", dict(subme=9, rd=63 | 64, trellis=127), 6)):
            out.append(_row(f"{ME_NAMES[m]}-{tag}", "b", "IBBP", dict(over, me_method=m), I=mb_id(2, 1, False, rd), P=mb_id(5, m, True, rd), B=mb_id(5, m, True, rd, True),
                            seed=50 + 3 * m + rd))
    # ---- psy-trellis and noise reduction: five sessions per search method reach the ten kernels of P and B slices (psy: and the four of I slices) ----
    levels = (("subme6", dict(subme=6), 2, 3, 7), ("trellis1", {}, 2, 3, 3), ("trellis2", dict(trellis=127), 2, 4, 4),
              ("refine", dict(subme=9, rd=63), 5, 5, 5), ("refine-trellis2", dict(subme=9, rd=63 | 64, trellis=127), 5, 6, 6))
    for m in (1, 2):
        for tag, over, M, rd_ip, rd_b in levels:
            out.append(_row(f"psy-{ME_NAMES[m]}-{tag}", "b", "IBBP", dict(over, me_method=m, psy_trellis_q8=PSY_TRELLIS_Q8), I=mb_id(2, 1, False, rd_ip, False, True),
                            P=mb_id(M, m, True, rd_ip, False, True), B=mb_id(M, m, True, rd_b, True, True), seed=60 + 5 * m + rd_b))
    for m in (1, 2):
        for tag, over, M, rd_ip, rd_b in levels:
            out.append(_row(f"nr-{ME_NAMES[m]}-{tag}", "nr", "IPBBP", dict(over, me_method=m), P=mb_id(M, m, True, rd_ip, False, False, True),
                            B=mb_id(M, m, True, rd_b, True, False, True), seed=80 + 5 * m + rd_b, nr=True))
    return out


ROWS = _rows()
BY_NAME = {r["name"]: r for r in ROWS}
assert len(BY_NAME) == len(ROWS)
ALL_IDS = frozenset(i for r in ROWS for i in r["ids"].values())
SLICE_OF = {"I": 2, "P": 0, "B": 1}          # x264gpu_pic.slice_type


def row_of_id(i):
    """the first row that pins an id"""
    return next(r["name"] for r in ROWS if i in r["ids"].values())


def frames_of(row):
    return synth_frames(W, H, len(row["types"]), seed=row["seed"])


def config_kw(row):
    """what the row hands tests/oracle_lib.default_config (the toolset import is late: test_gpu_bframes needs no GPU to import, but this module promises none)"""
    if row["harness"] == "ip":
        return dict(row["over"])
    from test_gpu_bframes import MEDIUM
    return dict(MEDIUM, **row["over"])

"""-m gpu: every compiled instantiation of the macroblock loop (k_mb.hip.h k_mb_slice<M, ME, PS, RD, BS, PSY, NR>; 103 separately compiled kernels) is launched
by a named row of tests/mb_instantiations.py, proven to have been launched (x264gpu_mb_kernels_seen) and compared bit for bit with the checker: records, levels,
reconstruction, CABAC context variables, and for rows with B pictures the host writer's stream through the checker's decoder (test_gpu_bframes.run).

Noise reduction: the checker has none.  An NR row's reference is the plain kernel of the same tuple, which the same table pins to the checker: with zero offsets
the NR kernels code what the plain ones code and gather statistics; with the offsets a session grows (x264gpu_nr_update behind every picture) the device's stream
decodes on the checker to the device's reconstruction.

tests/test_mb_instantiations_cpu.py holds the table against the sources and shows on the checker that no row is vacuous."""
import ctypes as C

import numpy as np
import pytest

import mb_instantiations as T
import oracle_lib as O

pytestmark = pytest.mark.gpu

SEEN_BY_ROWS = set()          # the union over the rows run so far (test_the_rows_launch_the_whole_table)


def seen(lib, reset):
    ids = (C.c_uint32 * 256)()
    n = lib.x264gpu_mb_kernels_seen(ids, 256, int(reset))
    assert 0 <= n <= 256
    return set(ids[:n])


def claim(lib, row, what=None):
    """the kernels launched since the last reset hold every id the row claims (of the slice types `what`); the set is emptied"""
    got = seen(lib, True)
    SEEN_BY_ROWS.update(got)
    want = {i for st, i in row["ids"].items() if what is None or st in what}
    assert want <= got, (f"row {row['name']} claims {[T.id_name(i) for i in sorted(want - got)]}, which it did not launch; launched: "
                         f"{[T.id_name(i) for i in sorted(got)]}")
    return got


def run_ip(row):
    """test_gpu_pipeline's per-picture comparison, with the context variables where the session carries them (test_pipeline_cabac_rd_bitexact)"""
    from gpu_enc import GpuEncoder
    from test_gpu_pipeline import CABAC_CTX_I, CABAC_CTX_P, compare
    kw = T.config_kw(row)
    cfg = O.default_config(T.W, T.H, **kw)
    og, gg = O.OracleEncoder(cfg), GpuEncoder(cfg)
    for i, f in enumerate(T.frames_of(row)):
        st = 2 if i == 0 else 0
        o_mb, o_lv = og.encode(f, st)
        g_mb, g_lv = gg.encode([f], st)
        compare(f"{row['name']} frame {i}", (T.W + 15) // 16, g_mb[0], o_mb, g_lv[0], o_lv, gg.recon(0), og.recon())
        if kw.get("cabac") and kw.get("rd"):
            used = CABAC_CTX_I if st == 2 else CABAC_CTX_P
            np.testing.assert_array_equal(gg.cabac_states(0, 0)[used], og.cabac_states()[used], err_msg=f"context variables after picture {i}")
    og.close(); gg.close()


def run_nr(lib, row):
    from test_gpu_nr import Session, _same_pictures, two_streams
    frames = two_streams(T.W, T.H, len(row["types"]), row["seed"])
    seen(lib, True)
    s = Session(lib, T.W, T.H, nr=False, **row["over"])
    plain = s.code(frames, row["types"])
    s.close()
    launched = seen(lib, True)
    assert not any(i & 1 for i in launched), f"the plain session launched NR kernels: {[T.id_name(i) for i in sorted(launched)]}"
    # zero offsets: the plain kernels' pictures, and statistics
    s = Session(lib, T.W, T.H, nr=True, **row["over"])
    zero = s.code(frames, row["types"])
    assert not s.offsets().any()
    s.close()
    claim(lib, row)
    _same_pictures(plain, zero, f"{row['name']}, zero offsets")
    for st, of_type in (("P", lambda pt: pt == 2), ("B", lambda pt: pt >= 3)):          # (picture types of bgop.schedule: 0 / 1 I, 2 P, 3 B reference, 4 B)
        assert any(p["sums"][x]["count"][c] for p in zero if of_type(p["pt"]) for x in range(2) for c in range(3)), f"no statistics from the {st} pictures"
    assert all(not any(p["sums"][x]["count"]) for p in zero if p["pt"] <= 1 for x in range(2)), "an I picture has none"
    # the offsets a session grows: the checker decodes what the device coded
    s = Session(lib, T.W, T.H, nr=True, **row["over"])
    pics = s.code(frames, row["types"], update=600, write=True)
    off = s.offsets()
    s.close()
    claim(lib, row)
    assert off[0].any() and off[1].any()
    dec = O.h264_decode(s.stream, len(pics), T.W, T.H)
    assert len(dec) == len(pics)
    for k, p in enumerate(pics):
        assert np.array_equal(dec[k], p["recon"][0]), f"picture {k} of the device's stream decodes differently"
    assert any(a["lv"].tobytes() != b["lv"].tobytes() for a, b in zip(pics, plain)), "the offsets move no level"


@pytest.mark.parametrize("name", [r["name"] for r in T.ROWS])
def test_row_is_bitexact_and_launches_its_kernels(gpu, name):
    row = T.BY_NAME[name]
    if row["harness"] == "nr":
        run_nr(gpu, row)
        return
    seen(gpu, True)
    if row["harness"] == "ip":
        run_ip(row)
    else:
        from test_gpu_bframes import run
        run(gpu, T.W, T.H, row["types"], row["seed"], frames=T.frames_of(row), **row["over"])
    got = claim(gpu, row)
    assert len(got) == len(row["ids"]), f"row {name} launched kernels it does not claim: {[T.id_name(i) for i in sorted(got)]}"


def test_the_rows_launch_the_whole_table(gpu):
    """after the rows (pytest runs a file's tests in the order they are written): every instantiation has been launched by the row that names it.  Run alone, this
    test walks the rows itself."""
    if not T.ALL_IDS <= SEEN_BY_ROWS:
        for r in T.ROWS:
            test_row_is_bitexact_and_launches_its_kernels(gpu, r["name"])
    assert SEEN_BY_ROWS >= T.ALL_IDS, f"never launched: {[T.id_name(i) for i in sorted(T.ALL_IDS - SEEN_BY_ROWS)]}"
    plain_of_nr = {i & ~1 for i in T.ALL_IDS if i & 1}          # the plain runs of the NR rows launch the NR kernels' plain twins
    assert SEEN_BY_ROWS <= T.ALL_IDS and plain_of_nr <= T.ALL_IDS, f"launched but not in the table: {[T.id_name(i) for i in sorted(SEEN_BY_ROWS - T.ALL_IDS)]}"

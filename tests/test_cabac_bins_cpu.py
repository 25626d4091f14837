"""CPU: the bin-by-bin restatement of the macroblock layer's own bins (tests/cabac_bins_ref.py, over cabac_levels_ref.step and the generated entropy table) that
the device's per-context bin strings are checked against through the primitive x264gpu_cabac_bins_walk agrees with the checker's state machine
(oracle/cabac_rd.cpp x264o_cabac_mb) on a handful of macroblocks whose bins are typed out by hand here: a skipped one, a P 16x16 with zero and with long vector
differences (escape suffix), an Intra_4x4 with sixteen predicted modes, an Intra_16x16 with a negative mb_qp_delta — bitstream order and size order."""
import ctypes as C

import numpy as np
import pytest

import cabac_bins_ref as R
import oracle_lib as O


class Ctx(C.Structure):
    _fields_ = [("mbs", C.c_void_p), ("levels", C.c_void_p), ("mbw", C.c_int), ("mbh", C.c_int), ("first_row", C.c_int), ("pslice", C.c_int), ("num_ref", C.c_int),
                ("t8mode", C.c_int), ("amvd", C.c_void_p), ("state", C.c_void_p), ("last_dqp", C.c_int), ("last_qp", C.c_int), ("bslice", C.c_int),
                ("num_ref1", C.c_int), ("amvd1", C.c_void_p)]


O.L.x264o_cabac_mb.argtypes = [C.POINTER(Ctx), C.c_int, C.c_int, C.c_int]
O.L.x264o_cabac_mb.restype = C.c_long
O.L.x264o_cabac_init_states.argtypes = [C.c_void_p, C.c_int, C.c_int]
O.L.x264o_cabac_init_states.restype = None

CBP0 = [(73, 0, 1), (74, 0, 1), (75, 0, 1), (76, 0, 1), (77, 0, 1)]          # coded_block_pattern 0 of a macroblock without neighbours


def _mb(**kw):
    m = np.zeros(1, O.MB_DTYPE)
    m["qp"] = 26
    m["ref"] = -1
    for k, v in kw.items():
        m[k] = v
    return m


P16 = [(11, 0, 1), (14, 0, 1), (15, 0, 1), (16, 0, 1)]
CASES = {
    # name: (pslice, record, size order?, the bins, bypass bins + the terminate bin's 7 / 256)
    "p_skip": (1, _mb(type=O.MB_P_SKIP), 0, [(11, 1, 1)], 0),
    "p16_zero_mvd": (1, _mb(type=O.MB_P_L0, ref=[[0, 0, 0, 0]]), 0, P16 + [(40, 0, 1), (47, 0, 1)] + CBP0, 0),
    # mvd 5: prefix 1 1 1 1 1 0 on 40, 43, 44, 45, 46, 46 + sign; mvd -12: 1 on 47, 50, 51, 52, five times 53, then Exp-Golomb order 3 of 3 (four bins) + sign
    "p16_long_mvd": (1, _mb(type=O.MB_P_L0, ref=[[0, 0, 0, 0]], mv=[[[5, -12]] * 4]), 0,
                     P16 + [(40, 1, 1), (43, 1, 1), (44, 1, 1), (45, 1, 1), (46, 1, 1), (46, 0, 1), (47, 1, 1), (50, 1, 1), (51, 1, 1), (52, 1, 1), (53, 1, 5)] + CBP0, 256 * 6),
    "p16_long_mvd_size": (1, _mb(type=O.MB_P_L0, ref=[[0, 0, 0, 0]], mv=[[[5, -12]] * 4]), 1,
                          P16[1:] + [(40, 1, 1), (43, 1, 1), (44, 1, 1), (45, 1, 1), (46, 1, 1), (46, 0, 1), (47, 1, 1), (50, 1, 1), (51, 1, 1), (52, 1, 1), (53, 1, 5)] + CBP0, 256 * 6),
    # every block's mode is the predicted one (DC, nothing around): sixteen ones on 68, none on 69
    "i4x4_all_predicted": (0, _mb(type=0, i4_mode=[[2] * 16], chroma_mode=1), 0, [(3, 0, 1), (68, 1, 16), (64, 1, 1), (67, 0, 1)] + CBP0, 0),
    # mb_qp_delta -3 = value 6: 1 on 60, 1 on 62, four ones and the zero on 63; the DC block's coded_block_flag with both neighbours missing (intra: 1 + 2)
    "i16x16_dqp": (0, _mb(type=2, i16_mode=3, chroma_mode=2, qp=23), 1,
                   [(3, 1, 1), (6, 0, 1), (7, 0, 1), (9, 1, 1), (10, 1, 1), (64, 1, 1), (67, 1, 1), (67, 0, 1), (60, 1, 1), (62, 1, 1), (63, 1, 4), (63, 0, 1), (88, 0, 1)], 7),
}


@pytest.mark.parametrize("name", list(CASES))
def test_restatement_agrees_with_the_checkers_state_machine(name):
    pslice, mb, size, triples, extra = CASES[name]
    st = np.zeros(460, np.uint8)
    O.L.x264o_cabac_init_states(st.ctypes.data, pslice, 26)
    before = st.tolist()
    lv = np.zeros(O.MB_LEVELS, np.int16)
    amvd, amvd1 = np.zeros(8, np.uint8), np.zeros(8, np.uint8)
    c = Ctx(mb.ctypes.data, lv.ctypes.data, 1, 1, 0, pslice, 1, 0, amvd.ctypes.data, st.ctypes.data, 0, 26, 0, 1, amvd1.ctypes.data)
    bits = O.L.x264o_cabac_mb(C.byref(c), 0, 0, size)
    want_st, want_bits = R.code(triples, before)
    assert st.tolist() == want_st
    assert bits == want_bits + extra


def test_runs_equal_single_bins_and_cases_are_reproducible():
    a, b = R.cases(300, 5), R.cases(300, 5)
    assert a == b
    for t, s in a[:120]:
        assert R.code(t, s) == R.code(R.one_by_one(t), s)

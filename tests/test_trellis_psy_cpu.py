"""psy-trellis on the CPU: (1) the pure-Python twin of the trellis search (tests/trellis_psy_ref.py) equals oracle/trellis.cpp at strength 0 and with the psy term, block for
block — what makes it the yardstick of the device's psy search (tests/test_gpu_psy_trellis.py); (2) the host's rules for --psy-rd a:b (x264
validate_parameters: clip, silent zero without psy / trellis, the chroma quantiser offset), over the host-over-oracle stub."""
import ctypes as C

import numpy as np
import pytest

import oracle_lib as O
import trellis_psy_ref as T

O.L.x264o_quant_trellis_cabac.argtypes = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p]
O.L.x264o_quant_trellis_cabac.restype = C.c_int


def _oracle(cat, qp, intra, coefs_scan, states):
    nc, zz = T.ncoef(cat), np.array(T.zigzag(cat))
    mf = np.array(T.mf_raster(cat, qp), np.uint16)
    want = np.zeros_like(coefs_scan)
    for b in range(len(coefs_scan)):
        raster = np.zeros(nc, np.int16)
        raster[zz] = coefs_scan[b]
        O.L.x264o_quant_trellis_cabac(raster.ctypes.data, mf.ctypes.data, qp, cat, intra, states.ctypes.data)
        want[b] = raster[zz]
    return want


blocks, states = T.random_blocks, T.random_states


@pytest.mark.parametrize("qp", [20, 26, 37, 51])
@pytest.mark.parametrize("intra", [0, 1])
@pytest.mark.parametrize("cat", [0, 1, 2, 3, 4, 5])
def test_twin_equals_oracle_at_strength_0(cat, intra, qp):
    rng = np.random.default_rng(9000 + 100 * cat + 2 * qp + intra)
    for kind in ("dense", "sparse", "zero", "escape"):
        nblk = 6 if cat == 5 else 16
        coefs, st = blocks(cat, qp, kind, nblk, rng), states(rng)
        guess = np.array([[((T.scan_tables(cat, qp)[1][i] + abs(int(c))) * T.scan_tables(cat, qp)[0][i]) >> 16 for i, c in enumerate(row)] for row in coefs])
        if cat in (1, 4):
            guess[:, 0] = 0
        if kind == "sparse": assert guess.max() == 1
        if kind == "zero": assert guess.max() == 0
        if kind == "escape": assert guess.max() >= 15
        want = _oracle(cat, qp, intra, coefs, st)
        got, got_nz = T.quant_trellis_blocks(coefs, cat, qp, intra, st)
        bad = np.nonzero((got != want).any(axis=1))[0]
        assert len(bad) == 0, f"{kind}: block {bad[0]} coefs {coefs[bad[0]].tolist()} twin {got[bad[0]].tolist()} oracle {want[bad[0]].tolist()}"
        # a fenc_dct without a strength changes nothing
        got2, _ = T.quant_trellis_blocks(coefs, cat, qp, intra, st, 0, rng.integers(-4000, 4000, coefs.shape))
        assert np.array_equal(got2, got)
        if kind == "dense":
            assert np.count_nonzero(want) > nblk


@pytest.mark.parametrize("psy", [38, 640])
@pytest.mark.parametrize("qp,intra", [(0, 1), (26, 0), (51, 1)])
@pytest.mark.parametrize("cat", [0, 1, 2, 3, 4, 5])
def test_twin_equals_oracle_with_the_psy_term(cat, qp, intra, psy):
    """oracle/trellis.cpp's own psy-trellis term (x264o_quant_trellis_cabac_psy: what the checker's macroblock loop runs under cfg.psy_trellis_q8, and
    so what whole pictures of the device are compared with) against the twin, block for block, in every category and kind of input"""
    f = O.L.x264o_quant_trellis_cabac_psy
    f.argtypes, f.restype = [C.c_void_p, C.c_void_p, C.c_int, C.c_int, C.c_int, C.c_void_p, C.c_int, C.c_void_p], C.c_int
    rng = np.random.default_rng(7000 + 100 * cat + 2 * qp + intra + psy)
    nc, zz = T.ncoef(cat), np.array(T.zigzag(cat))
    mf = np.array(T.mf_raster(cat, qp), np.uint16)
    moved = 0
    for kind in ("dense", "sparse", "escape"):
        coefs, st = blocks(cat, qp, kind, 6 if cat == 5 else 16, rng), states(rng)
        fenc = rng.integers(-12000, 12001, coefs.shape).astype(np.int16) if cat == 5 else rng.integers(-4500, 4501, coefs.shape).astype(np.int16)
        want, _ = T.quant_trellis_blocks(coefs, cat, qp, intra, st, psy, fenc)
        for b in range(len(coefs)):
            raster, fr = np.zeros(nc, np.int16), np.zeros(nc, np.int16)
            raster[zz], fr[zz] = coefs[b], fenc[b]
            f(raster.ctypes.data, mf.ctypes.data, qp, cat, intra, st.ctypes.data, psy, fr.ctypes.data)
            assert raster[zz].tolist() == want[b].tolist(), f"{kind} block {b}: coefs {coefs[b].tolist()} fenc {fenc[b].tolist()} oracle {raster[zz].tolist()} twin {want[b].tolist()}"
        moved += not np.array_equal(want, T.quant_trellis_blocks(coefs, cat, qp, intra, st)[0])
    assert moved or cat in (0, 3, 4) or psy < 640


def test_twin_psy_term_moves_levels_only_in_luma_non_dc_blocks():
    """the twin's own reading of the rule: a large strength changes levels in categories 1, 2, 5 and nothing in 0, 3, 4; position 0 of a block whose
    guess leaves only that position (the DC-only shortcut) is untouched"""
    rng = np.random.default_rng(5)
    for cat in range(6):
        coefs, st = blocks(cat, 26, "dense", 12, rng), states(rng)
        fenc = rng.integers(-3000, 3000, coefs.shape)
        a, _ = T.quant_trellis_blocks(coefs, cat, 26, 1, st)
        b, _ = T.quant_trellis_blocks(coefs, cat, 26, 1, st, 640, fenc)
        assert (not np.array_equal(a, b)) == (cat in (1, 2, 5)), cat
    only0 = np.zeros((1, 16), np.int16); only0[0, 0] = 300
    assert np.array_equal(T.quant_trellis_blocks(only0, 2, 26, 1, st)[0], T.quant_trellis_blocks(only0, 2, 26, 1, st, 640, fenc[:1, :16])[0])


# ---- (2) the host's rules, over the host-over-oracle stub (a child process: the stub must not meet the real device library) ----
_CHILD = r"""
import ctypes as C, json, os, sys
os.environ["X264_HOST_STUB"] = "1"
sys.path.insert(0, sys.argv[1]); sys.path.insert(0, os.path.dirname(sys.argv[1]))
import host_lib as HL
H = HL.H
out = {}
for name, tune, opts in json.loads(sys.argv[2]):
    p = HL.Param()
    assert H.x264_param_default_preset(C.byref(p), b"medium", tune.encode() if tune else None) == 0
    p.i_width, p.i_height, p.i_csp = 64, 48, HL.X264_CSP_I420
    p.i_fps_num, p.i_fps_den = 25, 1
    for o in opts:
        k, eq, v = o.partition("=")
        assert H.x264_param_parse(C.byref(p), k.encode(), v.encode() if eq else None) == 0, o
    log = []
    cb = C.CFUNCTYPE(None, C.c_void_p, C.c_int, C.c_char_p, C.c_void_p)(lambda priv, lvl, fmt, va: log.append([lvl, fmt.decode(errors="replace").strip()]))
    p.pf_log = C.cast(cb, C.c_void_p).value
    p.i_log_level = 3
    h = H.x264_encoder_open_157(C.byref(p))
    assert h, name
    eff = HL.Param()
    H.x264_encoder_parameters(h, C.byref(eff))
    H.x264_encoder_close(h)
    out[name] = {"psy_trellis": eff.analyse.f_psy_trellis, "cqo": eff.analyse.i_chroma_qp_offset, "trellis": eff.analyse.i_trellis, "me": eff.analyse.i_me_method,
                 "warn": [m for lvl, m in log if lvl <= 1]}
print(json.dumps(out))
"""
_BASE = ["me=hex", "trellis=1", "subme=7", "qp=26"]
_CASES = [("off", None, _BASE + ["psy-rd=1.0:0"]), ("s015", None, _BASE + ["psy-rd=1.0:0.15"]), ("s025", None, _BASE + ["psy-rd=1.0:0.25"]),
          ("s99", None, _BASE + ["psy-rd=1.0:99"]), ("nopsy", None, _BASE + ["psy-rd=1.0:0.15", "no-psy"]),
          ("trellis0", None, ["me=hex", "trellis=0", "subme=7", "qp=26", "psy-rd=1.0:0.15"]),
          ("dia", None, ["me=dia", "trellis=1", "subme=7", "qp=26", "psy-rd=1.0:0.15"]), ("dia_off", None, ["me=dia", "trellis=1", "subme=7", "qp=26", "psy-rd=1.0:0"]),
          ("cavlc", None, _BASE + ["psy-rd=1.0:0.15", "no-cabac"]), ("subme5", None, ["me=hex", "trellis=1", "subme=5", "qp=26", "psy-rd=1.0:0.15"]),
          ("film", "film", ["qp=26"]), ("grain", "grain", ["qp=26"]), ("umh2", None, ["me=umh", "trellis=2", "subme=9", "qp=26", "psy-rd=1.0:0.7"])]


@pytest.fixture(scope="module")
def host():
    import json, os, subprocess, sys
    here = os.path.dirname(os.path.abspath(__file__))
    subprocess.check_call(["make", "-s", "-C", os.path.join(here, "stub")])
    r = subprocess.run([sys.executable, "-c", _CHILD, here, json.dumps(_CASES)], capture_output=True, text=True, timeout=300)
    assert r.returncode == 0, r.stderr[-3000:]
    return json.loads(r.stdout.strip().splitlines()[-1])


def _psy_warnings(c):
    return [m for m in c["warn"] if "psy-trellis" in m]


def test_host_reports_the_strength_and_lowers_the_chroma_offset(host):
    off, a, b = host["off"], host["s015"], host["s025"]
    assert off["psy_trellis"] == 0 and abs(a["psy_trellis"] - 0.15) < 1e-6 and abs(b["psy_trellis"] - 0.25) < 1e-6
    assert a["cqo"] == off["cqo"] - 1 and b["cqo"] == off["cqo"] - 2
    assert not _psy_warnings(off) and not _psy_warnings(a) and not _psy_warnings(b)
    assert host["s99"]["psy_trellis"] == 10.0 and host["s99"]["cqo"] == off["cqo"] - 2          # clipped to 0..10
    u = host["umh2"]
    assert abs(u["psy_trellis"] - 0.7) < 1e-6 and u["trellis"] == 2 and not _psy_warnings(u)


def test_host_drops_it_silently_without_psy_or_trellis(host):
    for name in ("nopsy", "trellis0"):
        assert host[name]["psy_trellis"] == 0 and not _psy_warnings(host[name]), name
    assert host["trellis0"]["cqo"] == host["off"]["cqo"]


def test_host_says_so_where_the_session_cannot_run_it(host):
    for name in ("dia", "cavlc", "subme5"):
        c = host[name]
        assert c["psy_trellis"] == 0 and len(_psy_warnings(c)) == 1, (name, c)
    assert host["dia"]["cqo"] == host["dia_off"]["cqo"]          # no extra chroma drop


def test_tunings_carry_their_strength(host):
    assert abs(host["film"]["psy_trellis"] - 0.15) < 1e-6 and not _psy_warnings(host["film"])
    assert abs(host["grain"]["psy_trellis"] - 0.25) < 1e-6 and not _psy_warnings(host["grain"])


def test_first_macroblock_source_gives_mostly_intra_16x16():
    """the picture of tests/test_gpu_psy_trellis.py::test_first_macroblocks_of_slices_use_their_source_transform on the CPU checker at strength 0 (the
    analysis runs before the final encode, so the device's decisions at strength 45 are these): at least half of the sixteen first macroblocks are
    Intra_16x16, the other types occur too, the twin gives the checker's levels for every block that test checks, and strength 45 moves some of them"""
    import test_gpu_psy_trellis as G
    frames = G.first_mb_frames()
    n16, moved, types = 0, 0, set()
    for s in range(2):
        c = G.first_mb_config(0)
        c.streams = 1
        mb, lv = O.OracleEncoder(c).encode(frames[s], O.SLICE_I)
        y = frames[s][:16 * G.MBW * 16 * G.MBH].reshape(16 * G.MBH, 16 * G.MBW)
        for m in range(G.MBH):
            t = int(mb[m]["type"])
            types.add(t); n16 += t == 2
            src = y[16 * m:16 * m + 16, :16]
            for (off, w0), (_, w45) in zip(G.expected_first_mb_levels(src, t, t == 1, 0), G.expected_first_mb_levels(src, t, t == 1, 45)):
                assert lv[m][off:off + len(w0)].tolist() == w0, (s, m, t, off)
                moved += w0 != w45
    assert n16 >= G.MBH and types == {0, 1, 2} and moved > 0, (n16, types, moved)

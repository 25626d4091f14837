"""The load balance of the lock-step batch (x264vfw_amd/csrc/encoder.hip k_balance; k_mb.hip.h codes stream k.perm[workgroup]): its numpy twin, and the one table
of content and cases that tests/test_balance_cases_cpu.py (what the checker makes of them) and tests/test_gpu_balance.py (device == checker, stream by stream,
at 515 and 1027 streams) both run.  No GPU import.

From 512 streams up workgroup n no longer codes stream n, so everything the macroblock loop reads or writes per stream must go through the permuted index.  A
batch whose streams all hold the same content cannot show a wrong one; here stream s, s + 1 and s + 16 never share a sequence, stream 0 and the last stream hold
the cheapest content there is (they lose their workgroups as soon as any time differs), and quantisers, direct modes, offsets and vectors differ per stream.

The checker's sessions are computed once a process and key (functools.lru_cache) and shared by both files; their arrays must not be written to."""
import ctypes as C
import functools

import numpy as np

import hard_content as HC
import oracle_lib as O
from synth import synth_frames

W, H = 64, 48          # 4 x 3 macroblocks: the suite's smallest picture that still holds inter, intra and skipped macroblocks
MBW, NMB = 4, 12
K = 16
S_DEFAULT = 515        # just past the threshold of 512, and odd: half = (S + 1) / 2 rounds
S_BIG = 1027           # more workgroups than the 1024 SIMDs: the half dealt backwards shares SIMDs with the first


# ---- k_balance in numpy ----
def perm_ref(wtime):
    """perm[workgroup] = stream: the streams ranked by (time descending, index ascending); the slower half = (S + 1) // 2 of them keeps that order, the faster half
    is dealt backwards behind it"""
    t = np.asarray(wtime, np.uint32)
    S = len(t)
    order = np.lexsort((np.arange(S), -t.astype(np.int64)))          # last key first: time descending, ties by index ascending
    half = (S + 1) // 2
    r = np.arange(S)
    perm = np.full(S, -1, np.int32)
    perm[np.where(r < half, r, half + (S - 1 - r))] = order
    return perm


PERM_COUNTS = (1, 2, 3, 64, 511, 512, 513, 1023, 1024, 1025, 2048, 2049, 8191, 8192)


def wtime_arrays(S):
    """name -> the time arrays of S streams that the primitive is held against perm_ref on"""
    rng = np.random.default_rng(1000 + S)
    a = np.arange(S, dtype=np.uint64)
    sat = np.where(rng.random(S) < 0.5, 0xffffffff, 0).astype(np.uint32)          # (the loop's counter saturates there)
    outlier = np.full(S, 70000, np.uint32)
    outlier[(S * 2) // 3] = 4000000
    return {
        "random32": rng.integers(0, 1 << 32, S, dtype=np.uint64).astype(np.uint32),
        "equal": np.full(S, 123456, np.uint32),
        "ties0123": rng.integers(0, 4, S).astype(np.uint32),
        "ascending": (1000 + 3 * a).astype(np.uint32),
        "descending": (0xffffffff - 5 * a).astype(np.uint32),
        "saturated": sat,
        "outlier": outlier,
    }


# ---- content: K sequences with the widest spread of work a picture (the balancer only moves streams whose times differ) ----
def flat(value):
    def gen(w, h, n, seed):
        return [np.full(w * h * 3 // 2, value, np.uint8) for _ in range(n)]
    gen.__name__ = f"flat{value}"
    return gen


def _synth(w, h, n, seed):
    return synth_frames(w, h, n, seed=seed)


def _sequences():
    """Two flat and static ones (the least work there is), the project's synthetic pan at four seeds, full-range noise (the most: the seed is one at which no
    macroblock of any P or B picture is skipped or direct at any of the case's quantisers), and what the suite has in between.  hard_content's checker2 and
    rails_ramp are NOT among them: a checkerboard that moves one sample a frame and a ramp under +-3 of noise predict so well that whole P and B pictures
    code no level at these quantisers (tests/test_balance_cases_cpu.py wants every sequence but the flat ones to code something in every picture, so that no
    two streams' right answers coincide); cells2_static and cells4 stand in their places."""
    from test_gpu_b_pred_reuse import fast_pan, noisy_pan, static_noise          # (imports without a GPU; its tests are marked)
    kinds = HC.KINDS
    return [("flat16", flat(16), 0), ("flat235", flat(235), 0),
            ("synth", _synth, 3), ("synth", _synth, 11), ("synth", _synth, 23), ("synth", _synth, 47),
            ("noise_full", HC.noise_full, 8), ("moving_edges", HC.moving_edges, 6), ("cells4_static", kinds["cells4_static"], 7), ("cells2_static", kinds["cells2_static"], 9),
            ("cells4", kinds["cells4"], 9), ("noisy_pan", noisy_pan, 10), ("static_noise", static_noise, 12), ("fast_pan", fast_pan, 13),
            ("moving_edges", HC.moving_edges, 31), ("noisy_pan", noisy_pan, 32)]


FLAT = (0, 1)          # the sequences that may code nothing
NOISE_FULL = 6


def seq_name(k):
    name, _, seed = _sequences()[k]
    return f"{k}:{name}/{seed}"


@functools.lru_cache(maxsize=None)
def seq_frames(k, n):
    _, gen, seed = _sequences()[k]
    fr = [np.ascontiguousarray(f, np.uint8) for f in gen(W, H, n, seed)]
    assert len(fr) == n and all(f.shape == (W * H * 3 // 2,) for f in fr)
    return fr


def seq_of(s, S):
    """the sequence of stream s of S: s, s + 1 and s + 16 never share one; the first and the last stream hold the flat ones"""
    return 0 if s == 0 else 1 if s == S - 1 else (5 * s + s // 16) % K


def batch_frames(S, n, disp):
    return [seq_frames(seq_of(s, S), n)[disp] for s in range(S)]


def _rec(og, mb, lv, **more):
    return dict(mb=mb, lv=lv, recon=og.recon(), **more)


# ---- I / P pictures through x264gpu_encode_frames ----
IP_KW = dict(HC.MEDIUM_IP, trellis=63, aq_mode=1, qp_i=22, qp_p=25)
IP_TYPES = (2, 0, 0, 2, 0, 0)          # I P P I P P: the second I and every P from the second on run permuted
IP_PERMUTED = (2, 3, 4, 5)


@functools.lru_cache(maxsize=None)
def ip_session(k):
    og = O.OracleEncoder(O.default_config(W, H, **IP_KW))
    out = []
    for f, st in zip(seq_frames(k, len(IP_TYPES)), IP_TYPES):
        mb, lv = og.encode(f, st)
        out.append(_rec(og, mb, lv, states=og.cabac_states()))
    og.close()
    return out


# ---- B pictures through x264gpu_encode_pictures, the headline toolset ----
def b_kw():
    from test_gpu_bframes import MEDIUM
    return dict(MEDIUM, aq_mode=1)


B_TYPES = "IBBBPBBBPBBBP"          # coded I P R b b P R b b P R b b: every one of P, B reference and b three times
B_WEIGHTP = 2


def kind_of(pt):
    """encode_core's history index of a picture type of bgop.schedule (0 / 1 I, 2 P, 3 B reference, 4 B)"""
    return 0 if pt <= 1 else pt - 1


def permuted_pictures(pts):
    """the coding positions that run permuted: every picture but the first of its kind"""
    seen, out = set(), []
    for k, pt in enumerate(pts):
        if kind_of(pt) in seen:
            out.append(k)
        seen.add(kind_of(pt))
    return out


def base_qp(pt):
    return 20 if pt <= 1 else 23 if pt == 2 else 25 if pt == 4 else 24


def stream_controls(s):
    return s % 3, s % 5, s & 1


def copy_pic(pic):
    q = type(pic)()
    C.memmove(C.byref(q), C.byref(pic), C.sizeof(pic))
    return q


def stream_pic(pic, k, pt, q3, q5, temporal):
    """stream's own copy of the planned picture k: its quantiser, on every second picture the float quantiser of a rate-controlled session, its direct mode"""
    q = copy_pic(pic)
    q.qp = base_qp(pt) + q3
    q.qpm = q.qp + (37 * q5) / 256.0 if k & 1 else 0.0          # (exact in a single float)
    if pt >= 3:
        q.direct_temporal, q.direct_auto = int(temporal), 1
    return q


def b_plan(types=B_TYPES):
    """the host's DPB model and the coding order of the case (the caller plans, codes and commits picture by picture)"""
    import bgop
    import host_lib as HL
    kw = b_kw()
    return bgop.HostDpb(HL, kw["refs"], 3, 1, weightp=B_WEIGHTP), bgop.schedule(types, 1)


@functools.lru_cache(maxsize=None)
def b_session(k, q3, q5, temporal):
    import bgop
    og = O.OracleEncoder(O.default_config(W, H, **b_kw()))
    dpb, order = b_plan()
    frames = seq_frames(k, len(B_TYPES))
    out = []
    for i, (disp, pt) in enumerate(order):
        pic, _ = dpb.plan(pt, disp, bgop.follow_of(order, i))
        mb, lv = og.encode_pic(frames[disp], stream_pic(pic, i, pt, q3, q5, temporal))
        out.append(_rec(og, mb, lv, pt=pt, states=og.cabac_states(), dscore=og.direct_scores() if pt >= 3 else None))
        dpb.commit()
    og.close(); dpb.close()
    return out


# ---- side rows (per-macroblock quantiser offsets, lookahead vectors), two P pictures after an I ----
SIDE_KW = dict(HC.MEDIUM_IP, trellis=63, qp_i=22, qp_p=25)
SIDE_TYPES = (2, 0, 0)


@functools.lru_cache(maxsize=None)
def side_rows(S):
    """([S][nmb] float offsets in -6..6, [S][nmb][2] int16 vectors in the lookahead's half-resolution units), distinct per stream"""
    rng = np.random.default_rng(77)
    off = (rng.integers(-6 * 256, 6 * 256 + 1, (S, NMB)) / np.float32(256)).astype(np.float32)
    mv = rng.integers(-12, 13, (S, NMB, 2)).astype(np.int16)
    assert len({o.tobytes() for o in off}) == S and len({m.tobytes() for m in mv}) == S
    return off, mv


@functools.lru_cache(maxsize=None)
def side_session(s, S):
    off, mv = side_rows(S)
    og = O.OracleEncoder(O.default_config(W, H, **SIDE_KW))
    out = []
    for f, st in zip(seq_frames(seq_of(s, S), len(SIDE_TYPES)), SIDE_TYPES):
        og.set_mb_qp_offsets(off[s])
        O.L.x264o_encoder_set_lowres_mvs(og.h, O.ptr(mv[s]))
        mb, lv = og.encode(f, st)
        out.append(_rec(og, mb, lv))
    og.close()
    return out


# ---- noise reduction (no checker: the balanced encoder against the one created with X264GPU_NO_BALANCE) ----
NR_ROW = "nr-hex-trellis1"          # of tests/mb_instantiations.py
NR_TYPES = "IPBBPBBP"               # I P B B P and one more mini-GOP (coded I P P R b P R b): every kind of inter picture has a second one, which runs permuted
NR_QPS = (20, 23, 25)
NR_STRENGTHS = (0, 100, 1000)       # dealt by s % 3; strength 0 grows no offset: those streams code what the plain kernels code


def nr_kw():
    import mb_instantiations as T
    from test_gpu_bframes import MEDIUM
    return dict(MEDIUM, **T.BY_NAME[NR_ROW]["over"])


@functools.lru_cache(maxsize=None)
def nr_plain_session(k):
    """the checker's session of the NR case's toolset: what its strength-0 streams must code"""
    import bgop
    import host_lib as HL
    kw = nr_kw()
    og = O.OracleEncoder(O.default_config(W, H, **kw))
    dpb, order = bgop.HostDpb(HL, kw["refs"], 3, 1, weightp=0), bgop.schedule(NR_TYPES, 1)
    frames = seq_frames(k, len(NR_TYPES))
    out = []
    for i, (disp, pt) in enumerate(order):
        pic, _ = dpb.plan(pt, disp, bgop.follow_of(order, i))
        pic.qp = bgop.pic_qp(pt, *NR_QPS)
        mb, lv = og.encode_pic(frames[disp], pic)
        out.append(_rec(og, mb, lv, pt=pt))
        dpb.commit()
    og.close(); dpb.close()
    return out


def b_keys(S):
    """the checker sessions of the B case at S streams: (sequence, s % 3, s % 5, s & 1) of every stream"""
    return [(seq_of(s, S),) + stream_controls(s) for s in range(S)]

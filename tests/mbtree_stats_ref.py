"""The twin of the macroblock-tree statistics file (x264's <stats>.mbtree) and of the second pass' plan under it: written from x264's algorithm
([x264-upstream] common/mc.c mbtree_fix8_pack / _unpack; encoder/ratecontrol.c init_pass2, get_qscale, get_diff_limited_q), independently of the host's C++.

  pack / unpack          the file's number format: big-endian 8.8 fixed point, truncation toward zero, saturation, NaN -> 0
  read_file / write_file records of one byte of slice type (P 0, B 1, I 2) + nmb words
  init_pass2_tree        the plan; with tree=False it is x264's plain init_pass2 (pinned against oracle/decide.py by the tests), with tree=True the RCEQ value is
                         the frame-duration term alone and rc->qcompress is 1
"""
import ctypes
import ctypes.util
import math

import numpy as np

_m = ctypes.CDLL(ctypes.util.find_library("m") or "libm.so.6")
_m.powf.restype = _m.log2f.restype = ctypes.c_float
_m.powf.argtypes = [ctypes.c_float, ctypes.c_float]
_m.log2f.argtypes = [ctypes.c_float]
F = np.float32

SLICE_TYPE_P, SLICE_TYPE_B, SLICE_TYPE_I = 0, 1, 2
TYPE_OF_CHAR = {"I": SLICE_TYPE_I, "i": SLICE_TYPE_I, "P": SLICE_TYPE_P, "B": SLICE_TYPE_B}          # ('b' pictures have no record)


# ---- the number format ----
def pack(offsets):
    """float32 offsets -> the file's words as they lie on the wire (dtype '>i2')"""
    x = np.asarray(offsets, np.float32)
    with np.errstate(invalid="ignore", over="ignore"):
        v = x * F(256.0)                      # float32 multiply
        t = np.trunc(v)                       # toward zero
    t = np.where(np.isnan(t), F(0.0), t)
    return np.clip(t, -32768.0, 32767.0).astype(">i2")


def unpack(words):
    """the file's words (dtype '>i2', or raw bytes) -> float32 offsets"""
    w = np.frombuffer(words, ">i2") if isinstance(words, (bytes, bytearray)) else np.asarray(words, ">i2")
    return w.astype(np.float32) * F(1.0 / 256.0)


def record_size(nmb):
    return 1 + 2 * nmb


def read_file(path, nmb):
    """-> [(slice type byte, words '>i2')] in file order; the file must be whole records"""
    raw = open(path, "rb").read()
    rs = record_size(nmb)
    assert len(raw) % rs == 0, (len(raw), rs)
    return [(raw[k * rs], np.frombuffer(raw[k * rs + 1:(k + 1) * rs], ">i2")) for k in range(len(raw) // rs)]


def write_file(path, records):
    with open(path, "wb") as f:
        for t, words in records:
            f.write(bytes([t]) + np.asarray(words, ">i2").tobytes())


def kept_lines(stat_lines):
    """the statistics lines of the pictures kept as references, coding order: [(out, in, type char)]"""
    ent = []
    for ln in stat_lines:
        if ln.startswith("#") or not ln.strip():
            continue
        kv = dict(x.split(":", 1) for x in ln.split() if ":" in x)
        ent.append((int(kv["out"]), int(kv["in"]), kv["type"]))
    return [e for e in sorted(ent) if e[2] != "b"]


# ---- the second pass' plan ----
def _qp2qscale(qp):
    return float(F(0.85) * F(_m.powf(2.0, float((F(qp) - F(12.0)) / F(6.0)))))


def _qscale2qp(qs):
    return float(F(12.0) + F(6.0) * F(_m.log2f(float(F(qs) / F(0.85)))))


class Entry:
    """one line of the statistics: attribute names as oracle/decide.py's entries have them, so that its feedback replay (pass2_quantisers) takes these too"""

    def __init__(self, line):
        kv = dict(x.split(":", 1) for x in line.split() if ":" in x)
        self.frame, self.out, self.type = int(kv["in"]), int(kv["out"]), kv["type"]
        self.qscale = _qp2qscale(float(F(float(kv["q"]))))
        self.tex, self.mv, self.misc, self.icount = int(kv["tex"]), int(kv["mv"]), int(kv["misc"]), int(kv["imb"])
        self.kind = {"I": 0, "i": 0, "P": 1}.get(self.type, 2)
        self.kept_as_ref = self.type != "b"
        self.blurred = self.new_qscale = self.expected_bits = 0.0


def bits_at(e, qscale):
    """qscale2bits"""
    qscale = max(qscale, 0.1)
    return (e.tex + .1) * math.pow(e.qscale / qscale, 1.1) + e.mv * math.pow(max(e.qscale, 1) / max(qscale, 1), 0.5) + e.misc


def init_pass2_tree(lines, nmb, kbps, qcomp=0.6, fps=25.0, bframes=3, qblur=0.5, cplxblur=20.0, ip_factor=1.4, pb_factor=1.3, qpmin=0, qpmax=51, qpstep=4, tree=True):
    E = {}
    for ln in lines:
        if not ln.startswith("#") and ln.strip():
            e = Entry(ln)
            E[e.frame] = e
    n = len(E)
    E = [E[i] for i in range(n)]
    qcomp_param = float(F(qcomp))
    rc_qcompress = 1.0 if tree else qcomp_param          # x264_ratecontrol_new: rc->qcompress = 1 under b_mb_tree
    qblur, cplxblur = float(F(qblur)), float(F(cplxblur))
    ipf, pbf = abs(float(F(ip_factor))), abs(float(F(pb_factor)))
    dur = min(max(1.0 / fps, 0.01), 1.0) / 0.04          # CLIP_DURATION(frame duration) / BASE_FRAME_DURATION
    budget = kbps * 1000.0 * (n / fps)
    taps = int(qblur * 4) | 1
    base_cplx = nmb * (120 if bframes else 80)
    qstep = math.pow(2.0, qpstep / 6.0)
    lo, hi = _qp2qscale(qpmin), _qp2qscale(qpmax)
    assert budget >= sum(e.misc for e in E)

    def intra_share(e):
        return float(F(F(e.icount) / F(nmb))) ** 2

    # complexity blur (tree: computed as x264 does, never read)
    for i, e in enumerate(E):
        wsum = csum = 0.0
        w = 1.0
        for j in range(1, n - i):
            if not j < cplxblur * 2:
                break
            r = E[i + j]
            w *= 1 - intra_share(r)
            if w < .0001:
                break
            g = w * math.exp(-j * j / 200.0)
            wsum += g
            csum += g * (bits_at(r, 1) - r.misc) / dur
        w = 1.0
        for j in range(0, i + 1):
            if not j <= cplxblur * 2:
                break
            r = E[i - j]
            g = w * math.exp(-j * j / 200.0)
            wsum += g
            csum += g * (bits_at(r, 1) - r.misc) / dur
            w *= 1 - intra_share(r)
            if w < .0001:
                break
        e.blurred = float(F(csum / wsum))

    class S:
        pass
    s = S()

    def rceq(e):
        if tree:
            return math.pow(1.0 / dur, 1 - qcomp_param)          # BASE_FRAME_DURATION / CLIP_DURATION(duration), to the power 1 - qcomp
        return math.pow(e.blurred, 1 - rc_qcompress)

    def get_qscale(e, rate_factor):
        q = rceq(e)
        if not math.isfinite(q) or e.tex + e.mv == 0:
            return s.last_q[e.kind]
        return q / rate_factor

    def diff_limited(e, q):
        k = e.kind
        last_p_q = s.last_q[1]
        last_non_b_q = s.last_q[s.last_non_b] if s.last_non_b >= 0 else q
        if k == 0:
            iq = q
            if s.acc_norm <= 0:
                q = iq
            elif ip_factor < 0:
                q = iq / ipf
            else:
                pq = _qp2qscale(s.acc_qp / s.acc_norm)
                q = pq / ipf if s.acc_norm >= 1 else s.acc_norm * pq / ipf + (1 - s.acc_norm) * iq
        elif k == 2:
            if pb_factor > 0:
                q = last_non_b_q
            if not e.kept_as_ref:
                q *= pbf
        elif s.last_non_b == 1 and e.tex == 0:
            q = last_p_q
        if s.last_non_b == k and (k != 0 or s.last_acc_norm < 1):
            q = min(max(q, s.last_q[k] / qstep), s.last_q[k] * qstep)
        s.last_q[k] = q
        if k != 2:
            s.last_non_b = k
        if k == 0:
            s.last_acc_norm, s.acc_norm, s.acc_qp = s.acc_norm, 0.0, 0.0
        if k == 1:
            mask = float(F(1 - intra_share(e)))
            s.acc_qp = mask * (_qscale2qp(q) + s.acc_qp)
            s.acc_norm = mask * (1 + s.acc_norm)
        return q

    expected = 1.0
    s.last_q = [math.pow(base_cplx, 1 - rc_qcompress)] * 3
    for e in E:
        q = get_qscale(e, 1.0)
        expected += bits_at(e, q)
        s.last_q[e.kind] = q
    mult = budget / expected
    rf, step = 0.0, 1E4 * mult
    while step > 1E-7 * mult:
        expected = 0.0
        rf += step
        s.last_non_b, s.last_acc_norm, s.acc_norm, s.acc_qp = -1, 1.0, 0.0, 0.0
        s.last_q = [math.pow(base_cplx, 1 - rc_qcompress) / rf] * 3
        qs = []
        for e in E:
            qs.append(get_qscale(e, rf))
            s.last_q[e.kind] = qs[-1]
        for i in reversed(range(n)):
            qs[i] = diff_limited(E[i], qs[i])
        if taps > 1:
            sm = []
            for i in range(n):
                acc = wacc = 0.0
                for j in range(taps):
                    idx = i + j - taps // 2
                    d = idx - i
                    c = 1.0 if qblur == 0 else math.exp(-d * d / (qblur * qblur))
                    if 0 <= idx < n and E[idx].kind == E[i].kind:
                        acc += qs[idx] * c
                        wacc += c
                sm.append(acc / wacc)
        else:
            sm = qs
        for e, q in zip(E, sm):
            e.new_qscale = min(max(q, lo), hi)
            expected += bits_at(e, e.new_qscale)
        if expected > budget:
            rf -= step
        step *= 0.5
    spent = 0.0
    for e in sorted(E, key=lambda x: x.out):
        e.expected_bits = spent
        spent += bits_at(e, e.new_qscale)
    return E

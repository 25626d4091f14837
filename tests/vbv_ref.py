"""The Python twin of the host encoder's VBV (host/ratecontrol.cpp; [x264-upstream] encoder/ratecontrol.c: clip_qscale, predict_size / update_predictor,
update_vbv_plan, update_vbv, the MinCR limit of x264_ratecontrol_start) on top of the single-pass rate control twin of oracle/decide.py.  Restated from memory
of upstream like that file; doubles and single floats where x264 has them (predictor_t is all floats, clip_qscale works in doubles, rate_estimate_qscale's q is a
float).  Constant frame rate: every cpb duration is 1 / fps.

Fed what a session saw — picture types, lookahead costs, planned lists, header bits, coded sizes and the quantiser each picture was finally coded with — it
returns what the session's rate control must have computed: the quantiser before and after clip_qscale, frame_size_planned, and the buffer fill around every
picture.  A B picture's quantiser is an input (it follows from its references' quantisers, which tests/test_decisions_cpu.py covers); its planned size, its
share of the predictors and of the buffer are computed here."""
import math
import os
import sys

sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "oracle"))
import decide as D  # noqa: E402
from decide import _f, qp2qscale, qscale2qp  # noqa: E402

# Table A-1: level_idc -> (MaxMBPS, MinCR)
LEVELS = {10: (1485, 2), 9: (1485, 2), 11: (3000, 2), 12: (6000, 2), 13: (11880, 2), 20: (11880, 2), 21: (19800, 2), 22: (20250, 2), 30: (40500, 2), 31: (108000, 4),
          32: (216000, 4), 40: (245760, 4), 41: (245760, 2), 42: (522240, 2), 50: (589824, 2), 51: (983040, 2), 52: (2073600, 2), 60: (4177920, 2), 61: (8355840, 2),
          62: (16711680, 2)}
PLAN_I, PLAN_P, PLAN_B = (0, 1), (2,), (3, 4)          # the hook's planned types: PIC_IDR, PIC_I / PIC_P / PIC_BREF, PIC_B


def clip(v, lo, hi):
    return lo if v < lo else hi if v > hi else v


class Predictor:
    def __init__(self, coeff):
        self.coeff_min, self.coeff, self.count, self.decay, self.offset = _f(coeff / 2), _f(coeff), _f(1.0), _f(0.5), _f(0.0)

    def size(self, q, var):
        return _f(_f(_f(self.coeff * _f(var)) + self.offset) / _f(_f(q) * self.count))

    def update(self, q, var, bits):
        q, var, bits, rng = _f(q), _f(var), _f(bits), _f(1.5)
        if var < 10:
            return
        old_coeff, old_offset = _f(self.coeff / self.count), _f(self.offset / self.count)
        new_coeff = max(_f(_f(_f(bits * q) - old_offset) / var), self.coeff_min)
        clipped = clip(new_coeff, _f(old_coeff / rng), _f(old_coeff * rng))
        new_offset = _f(_f(bits * q) - _f(clipped * var))
        if new_offset >= 0:
            new_coeff = clipped
        else:
            new_offset = _f(0.0)
        self.count, self.coeff, self.offset = _f(self.count * self.decay), _f(self.coeff * self.decay), _f(self.offset * self.decay)
        self.count, self.coeff, self.offset = _f(self.count + 1), _f(self.coeff + new_coeff), _f(self.offset + new_offset)


class VbvRateControl(D.RateControl):
    """decide.RateControl with VBV: maxrate / bufsize in bits (under --nal-hrd: the HRD's unscaled values), init as a fraction"""

    def __init__(self, p, maxrate, bufsize, init, level_idc, lookahead, nominal_maxrate_kbit, nominal_bufsize_kbit, filler=False, annexb=True):
        super().__init__(p)
        self.vbv_max_rate, self.buffer_size = float(maxrate), float(bufsize)
        self.buffer_rate = self.vbv_max_rate / p.fps
        self.single_frame_vbv = self.buffer_rate * 1.1 > self.buffer_size
        self.vbv_min_rate = self.abr and nominal_maxrate_kbit * 1000.0 <= p.bitrate
        self.cbr_decay = 1.0
        if self.abr:
            self.cbr_decay = 1.0 - self.buffer_rate / self.buffer_size * 0.5 * max(0.0, 1.5 - self.buffer_rate * p.fps / p.bitrate)
        self.buffer_fill_final = self.buffer_size * _f(init)
        self.pred = [Predictor(1.5), Predictor(1.0), Predictor(1.0)]          # I, P, B
        self.pred_b_from_p = Predictor(0.5)
        self.lookahead, self.nominal = lookahead, (nominal_maxrate_kbit, nominal_bufsize_kbit)
        self.mbps, self.mincr = LEVELS[level_idc]
        self.level_idc, self.filler, self.filler_overhead = level_idc, filler, 5 if annexb else 6
        self.last_satd, self.bframe_bits, self.nonb_satd = 0.0, 0.0, 0.0
        self.lmin, self.lmax = qp2qscale(p.qpmin), qp2qscale(p.qpmax)

    # x264_ratecontrol_start: update_vbv_plan and the MinCR limit
    def begin(self, overhead_bits):
        p = self.p
        self.buffer_fill = min(self.buffer_fill_final, self.buffer_size) - overhead_bits
        nmb = p.mbw * p.mbh
        if self.frames_done == 0:
            fr = 1.0 / (300 if self.level_idc >= 60 else 172)
            self.frame_size_maximum = 384 * 8 * max(float(nmb), fr * self.mbps) / self.mincr
        else:
            self.frame_size_maximum = 384 * 8 * (1.0 / p.fps) * self.mbps / self.mincr

    def clip_qscale(self, is_i, q, planned, bframes):
        p, q0 = self.p, q
        pt = self.pred[0 if is_i else 1]
        if self.last_satd > 0:
            dur = 1.0 / p.fps
            if self.lookahead:
                terminate = 0
                for _ in range(1000):
                    if terminate == 3:
                        break
                    fill = self.buffer_fill - pt.size(q, self.last_satd)
                    total = 0.0
                    fq = [0.0] * 3
                    fq[1] = q * p.ip_factor if is_i else q
                    fq[2] = fq[1] * p.pb_factor
                    fq[0] = fq[1] / p.ip_factor
                    j = 0
                    while 0 <= fill <= self.buffer_size:
                        total += dur
                        fill += self.vbv_max_rate * dur
                        if j >= len(planned):
                            break
                        t, satd = planned[j]
                        k = 0 if t in PLAN_I else 1 if t in PLAN_P else 2
                        fill -= self.pred[k].size(fq[k], satd)
                        j += 1
                    target = min(self.buffer_fill + total * self.vbv_max_rate * 0.5, self.buffer_size * 0.5)
                    if fill < target:
                        q *= 1.01
                        terminate |= 1
                        continue
                    target = clip(self.buffer_fill - total * self.vbv_max_rate * 0.5, self.buffer_size * 0.8, self.buffer_size)
                    if self.vbv_min_rate and fill > target:
                        q /= 1.01
                        terminate |= 2
                        continue
                    break
            else:
                if (not is_i or self.last_non_b_is_i) and self.buffer_fill / self.buffer_size < 0.5:
                    q /= clip(2.0 * self.buffer_fill / self.buffer_size, 0.5, 1.0)
                bits = pt.size(q, self.last_satd)
                max_fill = 2 if self.nominal[1] >= 5 * self.nominal[0] / p.fps else 1
                min_fill = 1 if self.single_frame_vbv else 2
                if bits > self.buffer_fill / max_fill:
                    qf = clip(self.buffer_fill / (max_fill * bits), 0.2, 1.0)
                    q /= qf
                    bits *= qf
                if bits < self.buffer_rate / min_fill:
                    q *= clip(bits * min_fill / self.buffer_rate, 0.001, 1.0)
                q = max(q0, q)
            if not is_i and not self.single_frame_vbv:
                nb = bframes
                bits = pt.size(q, self.last_satd)
                bbits = self.pred_b_from_p.size(q * p.pb_factor, self.last_satd)
                pbbits, bdur = bits, nb * dur
                if bbits * nb > bdur * self.vbv_max_rate:
                    nb, bdur = 0, 0.0
                pbbits += nb * bbits
                space = self.buffer_fill + (bdur + dur) * self.vbv_max_rate - self.buffer_size
                if pbbits < space:
                    q *= max(pbbits / space, bits / (0.5 * self.buffer_size))
                q = max(q0 / 2, q)
            bits = pt.size(q, self.last_satd)
            fmax = min(self.frame_size_maximum, max(self.buffer_fill, 0.001))
            if bits > fmax:
                q *= bits / fmax
            if not self.vbv_min_rate:
                q = max(q0, q)
        if self.lmin == self.lmax:
            return self.lmin
        return clip(q, self.lmin, self.lmax)

    def nonb_vbv(self, is_i, satd, planned, bframes):
        """rate_estimate_qscale for an I / P picture -> (integer quantiser, float quantiser, qp_novbv, frame_size_planned)"""
        p = self.p
        self.cplxsum = self.cplxsum * 0.5 + satd / self.dur_ratio
        self.cplxcount = self.cplxcount * 0.5 + 1.0
        if satd > 0:
            rceq = (1.0 / self.dur_ratio) ** (1.0 - p.qcomp) if p.mbtree else (self.cplxsum / self.cplxcount) ** (1.0 - self.qcompress)
            self.last_rceq = rceq
            q = _f(rceq / (self.wanted_bits_window / self.cplxr_sum if self.abr else self.rate_factor_constant))
        else:
            q = _f(self.last_qscale_for[0 if is_i else 1])
        self.last_satd = self.nonb_satd = float(satd)
        overflow = 1.0
        if self.abr and satd > 0 and not self.vbv_min_rate:
            time_done = self.frames_done / p.fps
            wanted_bits = time_done * p.bitrate
            if wanted_bits > 0:
                abr_buffer = 2 * p.rate_tolerance * p.bitrate * max(1.0, math.sqrt(time_done))
                overflow = clip(1.0 + (self.total_bits - wanted_bits) / abr_buffer, .5, 2.0)
                q = _f(q * overflow)
        if is_i and p.keyint > 1 and not self.last_non_b_is_i:
            q = _f(qp2qscale(self.accum_p_qp / self.accum_p_norm) / p.ip_factor)
        elif self.frames_done > 0:
            if self.abr:
                lo, hi = self.last_qscale_for[0 if is_i else 1] / self.lstep, self.last_qscale_for[0 if is_i else 1] * self.lstep
                if overflow > 1.1 and self.frames_done > 3:
                    hi *= self.lstep
                elif overflow < 0.9:
                    lo /= self.lstep
                q = _f(clip(q, lo, hi))
        elif not self.abr and self.qcompress != 1.0:
            q = _f(qp2qscale(p.crf) / p.ip_factor)
        qp_novbv = qscale2qp(q)
        q = _f(self.clip_qscale(is_i, q, planned, bframes))
        self.last_qscale_for[0 if is_i else 1] = q
        if self.frames_done == 0:
            self.last_qscale_for[1] = q * p.ip_factor
        planned_size = self.buffer_rate if self.single_frame_vbv else self.pred[0 if is_i else 1].size(q, self.last_satd)
        planned_size = min(planned_size, self.frame_size_maximum)
        qpf = clip(qscale2qp(q), p.qpmin, p.qpmax)
        self._accum(qpf, is_i)
        self.last_non_b_is_i = is_i
        self.frames_done += 1
        return clip(int(qpf + 0.5), 1, 51), qpf, qp_novbv, planned_size

    def b_vbv(self, qpf, qf_unclipped):
        """a B picture whose quantiser the session computed (qpf; qf_unclipped: before [qpmin, qpmax]) -> frame_size_planned"""
        self.last_satd = self.nonb_satd          # the list-1 reference's cost: the picture that closed the mini-GOP
        planned_size = min(self.pred[2].size(qp2qscale(qf_unclipped), self.last_satd), self.frame_size_maximum)
        self._accum(qpf, False)
        self.frames_done += 1
        return planned_size

    def end_vbv(self, bits, kind, qpf_final, bframes, last_minigop_b):
        """x264_ratecontrol_end: kind 'I' / 'P' / 'B'; -> (buffer fill behind the picture, size of the filler NAL unit)"""
        p, is_b = self.p, kind == "B"
        if self.abr:
            self.total_bits += bits
            self.cplxr_sum += bits * qp2qscale(self.qp_avg_rc(qpf_final)) / (self.last_rceq * (abs(p.pb_factor) if is_b else 1.0))
            self.wanted_bits_window += p.bitrate / p.fps
            self.cplxr_sum *= self.cbr_decay
            self.wanted_bits_window *= self.cbr_decay
        qs = qp2qscale(self.qp_avg_rc(qpf_final))
        if self.last_satd >= p.mbw * p.mbh:
            self.pred["IPB".index(kind)].update(qs, self.last_satd, bits)
        if is_b:
            self.bframe_bits += bits
            if last_minigop_b:
                self.pred_b_from_p.update(qs, self.last_satd, self.bframe_bits / max(bframes, 1))
                self.bframe_bits = 0.0
        self.buffer_fill_final -= bits
        if self.buffer_fill_final < 0:
            self.buffer_fill_final = 0.0
        self.buffer_fill_final += self.buffer_rate
        filler = 0
        if self.filler and self.buffer_fill_final > self.buffer_size:
            filler = max(int(math.ceil((self.buffer_fill_final - self.buffer_size) / 8.0)), self.filler_overhead)
            self.buffer_fill_final -= 8.0 * filler
        elif self.buffer_fill_final > self.buffer_size:
            self.buffer_fill_final = self.buffer_size
        return self.buffer_fill_final, filler


def replay(info, mbw, mbh):
    """info: what tests/stub/run_host_vbv.py reports of a session.  -> per picture {"qp", "qp_clipped", "qp_novbv", "frame_size_planned", "fill_before", "fill_after",
    "filler"} as the twin computes them (for a B picture "qp" / "qp_clipped" / "qp_novbv" are None: its quantiser is an input)"""
    e = info["eff"]
    abr = e["rc_method"] == 2
    p = D.Params(mbw, mbh, keyint=e["keyint"], bframes=e["bframes"], crf=e["crf"], qcomp=e["qcomp"], ip_factor=e["ipratio"], pb_factor=e["pbratio"], qpmin=e["qp_min"],
                 qpmax=e["qp_max"], fps=e["fps"][0] / e["fps"][1], mbtree=bool(e["mbtree"]), rc_lookahead=e["lookahead"], bitrate=e["bitrate"] if abr else 0,
                 rate_tolerance=e["ratetol"], qpstep=e["qpstep"])
    v0 = info["vbv"][0]
    rc = VbvRateControl(p, v0["max_rate"], v0["buffer_size"], e["vbv_init"], e["level"], e["lookahead"] > 0, e["vbv_maxrate"], e["vbv_bufsize"], filler=e["nal_hrd"] == 2)
    kinds = ["I" if r[0] in (1, 2) else "P" if r[0] == 3 else "B" for r in info["recs"]]
    out, n, minigop_b = [], len(kinds), 0
    for k, (r, v, d) in enumerate(zip(info["recs"], info["vbv"], info["decisions"])):
        kind = kinds[k]
        rc.begin(v["overhead_bits"])
        row = {"fill_before": rc.buffer_fill}
        if kind != "B":
            minigop_b = 0
            while k + 1 + minigop_b < n and kinds[k + 1 + minigop_b] == "B":
                minigop_b += 1
            qp, qpf, novbv, planned_size = rc.nonb_vbv(kind == "I", d[2][0] if kind == "I" else d[2][1], [tuple(x) for x in v["planned"]], minigop_b)
            row.update(qp=qp, qp_clipped=qpf, qp_novbv=novbv, frame_size_planned=planned_size)
            last_b = False
        else:
            row.update(qp=None, qp_clipped=None, qp_novbv=None, frame_size_planned=rc.b_vbv(v["qp_clipped"], v["qp_novbv"]))
            last_b = k + 1 == n or kinds[k + 1] != "B"
        row["fill_after"], row["filler"] = rc.end_vbv(8 * (r[4] - int(v["filler"])), kind, v["qp_final"], minigop_b, last_b)
        out.append(row)
    return out

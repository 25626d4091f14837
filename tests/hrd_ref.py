"""A reader of what an H.264 stream says about its hypothetical reference decoder, written from ITU-T H.264 alone: the NAL unit syntax of Annex B / 7.3.1, the
sequence parameter set with its VUI and hrd_parameters() (7.3.2.1, E.1.1, E.1.2), the buffering-period and picture-timing SEI messages (D.1.1 - D.1.3), the first
fields of a slice header (7.3.3), and the CPB / DPB timing of Annex C.1 / C.2 replayed from those values.  No encoder source was consulted."""
from fractions import Fraction


# ---- Annex B / 7.3.1 ----
def split_annexb(stream):
    """-> [(nal_ref_idc, nal_unit_type, rbsp bytes, bytes the NAL unit takes in the stream incl. its start code and the zero bytes in front of it)] in stream order"""
    starts, i, n = [], 0, len(stream)
    while i + 3 <= n:
        if stream[i] == 0 and stream[i + 1] == 0 and stream[i + 2] == 1:
            starts.append(i + 3)
            i += 3
        else:
            i += 1
    leads = []
    for k, s in enumerate(starts):          # leading_zero_8bits / zero_byte in front of a start code prefix belong to the NAL unit that follows
        lead = s - 3
        floor = starts[k - 1] if k else 0
        while lead > floor and stream[lead - 1] == 0:
            lead -= 1
        leads.append(lead)
    out = []
    for k, s in enumerate(starts):
        end = leads[k + 1] if k + 1 < len(starts) else n
        body = stream[s:end]
        rbsp, zeros = bytearray(), 0
        for b in body[1:]:                  # emulation_prevention_three_byte (7.3.1)
            if zeros >= 2 and b == 3:
                zeros = 0
                continue
            rbsp.append(b)
            zeros = zeros + 1 if b == 0 else 0
        out.append((body[0] >> 5 & 3, body[0] & 31, bytes(rbsp), end - (leads[k] if k else 0)))
    return out


class Bits:
    def __init__(self, data):
        self.d, self.pos = data, 0

    def u(self, n):
        v = 0
        for _ in range(n):
            v = v << 1 | (self.d[self.pos >> 3] >> (7 - (self.pos & 7)) & 1)
            self.pos += 1
        return v

    def ue(self):
        z = 0
        while self.u(1) == 0:
            z += 1
        return (1 << z) - 1 + (self.u(z) if z else 0)

    def se(self):
        k = self.ue()
        return (k + 1) // 2 if k & 1 else -(k // 2)

    def more_rbsp_data(self):
        """7.2: data left in front of rbsp_trailing_bits"""
        last = len(self.d) - 1
        while last >= 0 and self.d[last] == 0:
            last -= 1
        if last < 0:
            return False
        stop = last * 8 + 7 - ((self.d[last] & -self.d[last]).bit_length() - 1)          # position of the rbsp_stop_one_bit
        return self.pos < stop


# ---- E.1.2 ----
def parse_hrd(b):
    h = {"cpb_cnt": b.ue() + 1, "bit_rate_scale": b.u(4), "cpb_size_scale": b.u(4), "sched": []}
    for _ in range(h["cpb_cnt"]):
        rate, size, cbr = b.ue() + 1, b.ue() + 1, b.u(1)
        h["sched"].append({"bit_rate": rate << (6 + h["bit_rate_scale"]), "cpb_size": size << (4 + h["cpb_size_scale"]), "cbr_flag": cbr})          # (E-37), (E-38)
    h["initial_cpb_removal_delay_length"] = b.u(5) + 1
    h["cpb_removal_delay_length"] = b.u(5) + 1
    h["dpb_output_delay_length"] = b.u(5) + 1
    h["time_offset_length"] = b.u(5)
    return h


# ---- 7.3.2.1.1, E.1.1 ----
def parse_sps(rbsp):
    b = Bits(rbsp)
    s = {"profile_idc": b.u(8)}
    b.u(8)
    s["level_idc"] = b.u(8)
    s["sps_id"] = b.ue()
    if s["profile_idc"] in (100, 110, 122, 244, 44, 83, 86, 118, 128, 138, 139, 134, 135):
        cf = b.ue()
        if cf == 3:
            b.u(1)
        b.ue(); b.ue(); b.u(1)
        assert b.u(1) == 0, "scaling matrices are not read here"
    s["log2_max_frame_num"] = b.ue() + 4
    s["poc_type"] = b.ue()
    if s["poc_type"] == 0:
        s["log2_max_poc_lsb"] = b.ue() + 4
    elif s["poc_type"] == 1:
        b.u(1); b.se(); b.se()
        for _ in range(b.ue()):
            b.se()
    s["max_num_ref_frames"] = b.ue()
    b.u(1)
    s["mbw"], s["map_h"] = b.ue() + 1, b.ue() + 1
    s["frame_mbs_only"] = b.u(1)
    if not s["frame_mbs_only"]:
        b.u(1)
    b.u(1)
    if b.u(1):
        b.ue(); b.ue(); b.ue(); b.ue()
    s["vui"] = None
    if b.u(1):
        v = {}
        if b.u(1):
            if b.u(8) == 255:
                b.u(16); b.u(16)
        if b.u(1):
            b.u(1)
        if b.u(1):
            b.u(3); b.u(1)
            if b.u(1):
                b.u(8); b.u(8); b.u(8)
        if b.u(1):
            b.ue(); b.ue()
        v["timing"] = b.u(1)
        if v["timing"]:
            v["num_units_in_tick"], v["time_scale"], v["fixed_frame_rate"] = b.u(32), b.u(32), b.u(1)
        v["nal_hrd"] = parse_hrd(b) if b.u(1) else None
        v["vcl_hrd"] = parse_hrd(b) if b.u(1) else None
        if v["nal_hrd"] or v["vcl_hrd"]:
            v["low_delay_hrd_flag"] = b.u(1)
        v["pic_struct_present"] = b.u(1)
        if b.u(1):
            b.u(1); b.ue(); b.ue(); b.ue(); b.ue()
            v["max_num_reorder_frames"], v["max_dec_frame_buffering"] = b.ue(), b.ue()
        s["vui"] = v
    assert not b.more_rbsp_data(), "bits left in the SPS"
    return s


# ---- D.1.1: sei_rbsp -> [(payloadType, payload bytes)] ----
def parse_sei(rbsp):
    out, i = [], 0
    while True:
        t = 0
        while rbsp[i] == 0xFF:
            t += 255
            i += 1
        t += rbsp[i]
        i += 1
        n = 0
        while rbsp[i] == 0xFF:
            n += 255
            i += 1
        n += rbsp[i]
        i += 1
        out.append((t, rbsp[i:i + n]))
        i += n
        if rbsp[i:] == b"\x80":              # rbsp_trailing_bits: no more_rbsp_data()
            return out


def _payload_tail_ok(b):
    """D.1.1 sei_payload: bit_equal_to_one and zero bits up to the byte boundary when the payload does not end on one"""
    left = len(b.d) * 8 - b.pos
    return left == 0 or (left < 8 and b.u(1) == 1 and b.u(left - 1) == 0)


def parse_buffering_period(payload, sps):
    b = Bits(payload)
    hrd = sps["vui"]["nal_hrd"]
    r = {"sps_id": b.ue(), "initial_cpb_removal_delay": [], "initial_cpb_removal_delay_offset": []}
    for _ in range(hrd["cpb_cnt"]):
        r["initial_cpb_removal_delay"].append(b.u(hrd["initial_cpb_removal_delay_length"]))
        r["initial_cpb_removal_delay_offset"].append(b.u(hrd["initial_cpb_removal_delay_length"]))
    assert sps["vui"]["vcl_hrd"] is None and _payload_tail_ok(b)
    return r


def parse_pic_timing(payload, sps):
    b = Bits(payload)
    hrd = sps["vui"]["nal_hrd"]
    r = {"cpb_removal_delay": b.u(hrd["cpb_removal_delay_length"]), "dpb_output_delay": b.u(hrd["dpb_output_delay_length"])}
    assert not sps["vui"]["pic_struct_present"] and _payload_tail_ok(b)
    return r


# ---- 7.3.3 (first fields) ----
def parse_slice_start(rbsp, sps, nal_unit_type):
    b = Bits(rbsp)
    r = {"first_mb": b.ue(), "slice_type": b.ue() % 5, "pps_id": b.ue(), "frame_num": b.u(sps["log2_max_frame_num"])}
    if nal_unit_type == 5:
        r["idr_pic_id"] = b.ue()
    if sps["poc_type"] == 0:
        r["poc_lsb"] = b.u(sps["log2_max_poc_lsb"])
    return r


def access_units(stream):
    """-> (sps, [access unit]) with access unit = {"bytes": its size incl. start codes, "filler": bytes of its filler NAL units, "nal_types", "bp", "pt", "idr",
    "poc_lsb", "frame_num"}; a new access unit starts at the first NAL unit of type 9, 7, 8 or 6 behind a slice, or at a slice with first_mb 0 behind a slice (7.4.1.2.3,
    as far as these streams need it)"""
    sps, aus, cur, seen_slice = None, [], None, False

    def new_au():
        return {"bytes": 0, "filler": 0, "nal_types": [], "bp": None, "pt": None, "idr": False, "poc_lsb": None, "frame_num": None}
    for ref_idc, t, rbsp, nbytes in split_annexb(stream):
        first_slice = False
        if t in (1, 5):
            sl = parse_slice_start(rbsp, sps, t)
            first_slice = sl["first_mb"] == 0
        if cur is None or (seen_slice and (t in (6, 7, 8, 9) or first_slice)):
            cur = new_au()
            aus.append(cur)
            seen_slice = False
        cur["bytes"] += nbytes
        cur["nal_types"].append(t)
        if t == 7:
            sps = parse_sps(rbsp)
        elif t == 6:
            for pt, payload in parse_sei(rbsp):
                if pt == 0:
                    cur["bp"] = parse_buffering_period(payload, sps)
                elif pt == 1:
                    cur["pt"] = parse_pic_timing(payload, sps)
        elif t == 12:
            assert all(x == 0xFF for x in rbsp[:-1]) and rbsp[-1] == 0x80, "filler data: ff_byte x n, rbsp_trailing_bits (7.3.2.7)"
            cur["filler"] += nbytes
        elif t in (1, 5):
            seen_slice = True
            if first_slice:
                cur["idr"], cur["poc_lsb"], cur["frame_num"] = t == 5, sl.get("poc_lsb"), sl["frame_num"]
    return sps, aus


def replay(sps, aus, sched=0):
    """Annex C.1.1 / C.1.2 / C.2.2 from the SEI values alone, in exact fractions of a second.  -> per access unit {"t_ai", "t_af", "t_r" (nominal removal),
    "t_o" (output)}.  Every access unit must carry a picture-timing SEI, the first one a buffering-period SEI"""
    vui = sps["vui"]
    hrd = vui["nal_hrd"]
    s = hrd["sched"][sched]
    t_c = Fraction(vui["num_units_in_tick"], vui["time_scale"])          # (C-1)
    rate = s["bit_rate"]
    out, t_af_prev, t_r_bp = [], Fraction(0), None
    for n, au in enumerate(aus):
        assert au["pt"] is not None, f"access unit {n} has no picture-timing SEI"
        bits = 8 * au["bytes"]
        if n == 0:
            assert au["bp"] is not None, "the first access unit has no buffering-period SEI"
            t_r = Fraction(au["bp"]["initial_cpb_removal_delay"][sched], 90000)          # (C-7)
        else:
            t_r = t_r_bp + t_c * au["pt"]["cpb_removal_delay"]                           # (C-8): from the removal of the last buffering-period picture
        if n == 0:
            t_ai = Fraction(0)
        elif s["cbr_flag"]:
            t_ai = t_af_prev                                                           # (C-2)
        else:
            # (C-3), (C-4), (C-5): the first access unit of a buffering period may use the delay alone, the others delay + offset
            d = au["bp"]["initial_cpb_removal_delay"][sched] if au["bp"] else bp_last["initial_cpb_removal_delay"][sched] + bp_last["initial_cpb_removal_delay_offset"][sched]
            t_ai = max(t_af_prev, t_r - Fraction(d, 90000))
        t_af = t_ai + Fraction(bits, rate)                                              # (C-6)
        if au["bp"] is not None:
            t_r_bp, bp_last = t_r, au["bp"]
        out.append({"t_ai": t_ai, "t_af": t_af, "t_r": t_r, "t_o": t_r + t_c * au["pt"]["dpb_output_delay"], "bits": bits})          # (C-12)
        t_af_prev = t_af
    return out

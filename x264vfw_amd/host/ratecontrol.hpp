// ratecontrol.hpp — the host encoder's rate control ([x264-upstream] encoder/ratecontrol.c restated; checker twin: oracle/decide.py class RateControl, init_pass2,
// pass2_quantisers; the VBV part: tests/vbv_ref.py): constant quantiser with --ipratio / --pbratio and zones, single-pass CRF and ABR, both passes of a 2-pass encode,
// and the VBV of single-pass CRF / ABR sessions at picture level (clip_qscale, the size predictors, the buffer account; no row-level re-quantisation: the session
// codes a picture again instead, encoder.cpp).  One object per session behind x264's three calls — open, start for every picture about to be coded, end once its
// size is known; plain C++ over x264_param_t and numbers.
#pragma once
#include "host.hpp"
#include <stdio.h>
#include <vector>

namespace x264host {

struct RateControl {
    // which rate control the session runs (session policy: set by Settings::settle, host/settings.hpp, before open()); none: constant quantiser
    bool crf = false, abr = false;       // single pass: the quantisers follow the lookahead's frame costs (ABR: and the coded sizes)
    bool pass1 = false, pass2 = false;   // a statistics line per coded picture; every quantiser planned from the first pass' statistics
    // the macroblock-tree statistics file (host/mbtreestats.hpp; session policy as well): a first pass that writes it says so in the statistics' header; a second
    // pass that reads it plans with the tree's RCEQ
    bool tree_write = false, tree_read = false;
    bool by_cost() const { return crf || abr; }
    bool reads_sizes() const { return abr || pass1 || pass2 || vbv; }          // end() feeds start(): such a session codes one picture at a time
    // VBV (session policy as well: Settings::settle validates --vbv-maxrate / --vbv-bufsize / --vbv-init / --nal-hrd and leaves the effective values in the parameters)
    bool vbv = false, vbv_lookahead = false;          // vbv_lookahead: rc-lookahead > 0, every I / P picture comes with the planned types and costs of the pictures behind it
    bool filler = false;                              // --nal-hrd cbr: what the buffer cannot hold is sent as filler (end() says how many bytes)
    int hrd_rate = 0, hrd_size = 0;                   // --nal-hrd: the rate and size the HRD signals (value << scale: what is left of the request), which the VBV then runs on; 0: as asked
    int qp_constant[5] = { 23, 23, 23, 23, 23 };          // x264 rc->qp_constant[] by PIC_*: a constant-quantiser session's quantisers outside its zones

    struct Zone { int start, end; bool force_qp; int qp; float bitrate_factor; };      // x264_zone_t: pictures start..end (display order) at quantiser qp, or at bitrate_factor times their bits
    std::vector<Zone> zones;
    void parse_zones(const x264_param_t &p);          // --zones; what does not parse is said in the log and dropped

    // x264_ratecontrol_new: the single-pass state, the second pass' plan (statistics file, init_pass2), the statistics file to write and its header line.
    // false, said in the log: statistics unreadable, damaged or empty; bitrate too low for the plan
    bool open(const x264_param_t &p, int mbw, int mbh, int bframes, int qp_i, int qp_p);
    // x264_ratecontrol_start: the quantiser of the next picture in coding order — kind PIC_*, display index, the lookahead's sums ([0] intra, [1] inter: I / P pictures
    // under CRF / ABR), a B picture's nearest reference of each list (CRF / ABR): the DPB slot it was kept() in, its POC distance.  -> the integer quantiser; *qpf:
    // the float one (x264 rc->qpm before the macroblock offsets)
    struct BRefs { int slot[2], dpoc[2]; };
    int start(int kind, int frame, const int32_t costs[4] = nullptr, const BRefs *b = nullptr, double *qpf = nullptr);
    // VBV sessions, before start(): what x264 keeps on the frame — the planned types (PIC_*, PLAN_END behind the last) and costs of the pictures coded after this one
    // (vbv_lookahead in the slice-type analysis; nullptr: none), the B pictures of the mini-GOP it closes (or belongs to), whether it is the last B picture of its
    // mini-GOP, and the bits of the header NAL units already in its access unit
    enum { PLAN_MAX = 64, PLAN_END = -1 };
    struct Planned { int type[PLAN_MAX + 1] = { PLAN_END }; int satd[PLAN_MAX + 1] = { 0 }; };
    void vbv_picture(const Planned *planned, int bframes, bool last_minigop_b, long overhead_bits);
    // ... and what start() made of them: the buffer fill it saw, the quantiser before clip_qscale (x264 rc->qp_novbv), the planned size and the size limit
    double buffer_fill = 0, qp_novbv = 0, frame_size_planned = 0, frame_size_maximum = 0;
    double buffer_size = 0, vbv_max_rate = 0, buffer_rate = 0, buffer_fill_final = 0;          // bits, bits / s, bits a picture; the fill behind the last coded picture
    int qp_ceiling() const;          // the highest quantiser a picture may be coded again with (qpmax)
    void kept(int slot, double qpf, int kind);          // a picture kept as a reference went into DPB slot `slot` (x264 fdec->f_qp_avg_rc, i_type)
    // x264_ratecontrol_end: ABR's feedback, the second pass' account, the statistics line (st: needed for that line only)
    struct PicStats { long imb = 0, pmb = 0, smb = 0, mv_bits = 0, tex_bits = 0; double aq_mean = 0; char direct = '-'; };      // intra / inter / skipped macroblocks, header / residual bits, mean quantiser
    // -> the size of the filler NAL unit the access unit is to be padded with (--nal-hrd cbr under VBV; filler_overhead() of it is not payload), else 0
    int end(size_t bytes, int kind, int frame, double qpf, const PicStats *st = nullptr);
    int filler_overhead() const { return p->b_annexb ? 5 : 6; }          // start code (or length), NAL header, trailing bits
    void close();          // x264_ratecontrol_delete: the statistics file takes its name (a second pass that stopped short keeps the statistics it read)

    // the second pass' plan by display index (nullptr behind its end)
    struct Pass2Entry { char type = 'P'; int in = 0, out = 0, icount = 0, kept_as_ref = 1; double qscale = 0, new_qscale = 0, blurred = 0, expected_bits = 0, dur = 1;
                        long tex = 0, mv = 0, misc = 0; };
    const Pass2Entry *plan(int frame) const { return frame >= 0 && frame < (int)p2.size() ? &p2[(size_t)frame] : nullptr; }
    int planned() const { return (int)p2.size(); }

    int frames_done = 0;          // pictures start() has seen (coding order, B included); in I / P sessions and for GOP slots under CRF also the display index

private:
    const x264_param_t *p = nullptr;
    int mbw = 0, mbh = 0, nmb = 0;
    bool mbtree = false;
    // rate_estimate_qscale's state (doubles as in x264)
    double rate_factor_constant = 1, qcompress = 0.6, ip_factor = 1, pb_factor = 1, ip_offset = 0, pb_offset = 0, dur_ratio = 1, fps = 25;
    double cplxsum = 0, cplxcount = 0, accum_p_qp = 0, accum_p_norm = 0, lmin = 0, lmax = 0;
    double last_qscale_for[2] = { 0, 0 };       // [0] I, [1] P
    int last_non_b_is_i = 1;
    double bitrate = 0, cplxr_sum = 0, wanted_bits_window = 0, abr_buffer = 0, total_bits = 0, last_rceq = 1, lstep = 1.3195;      // single-pass ABR
    double slot_qp_rc[8] = { 0 }; int slot_kind[8] = { 0 };          // kept(): by DPB slot
    // VBV (x264's predictor_t: single floats)
    struct Predictor { float coeff_min, coeff, count, decay, offset; };
    Predictor pred[3] = {}, pred_b_from_p = {};          // [0] I, [1] P, [2] B
    bool vbv_min_rate = false, single_frame_vbv = false;
    double cbr_decay = 1.0, last_satd = 0, bframe_bits = 0, slot_satd[8] = { 0 };
    const Planned *cur_planned = nullptr; int cur_bframes = 0; bool cur_last_b = false; long cur_overhead = 0;
    int level_mbps = 0, level_mincr = 2;
    static double predict_size(const Predictor &p, double q, double var);
    static void update_predictor(Predictor &p, double q, double var, double bits);
    double clip_qscale(bool is_i, double q);
    // 2-pass: the statistics file being written (a line per coded picture); the plan init_pass2 made from the one read, followed with feedback
    FILE *stat_file = nullptr;
    std::vector<Pass2Entry> p2;          // by display index ("in:")
    std::vector<int> p2_out;             // coding order -> display index
    double p2_expected_sum = 0, p2_total_bits = 0, p2_final_bits = 0, p2_abr_buffer = 0;
    long coded = 0;                      // pictures end() has seen

    const Zone *get_zone(int frame) const;
    double pick_qp(bool is_i, const int32_t costs[4], int frame);
    double pick_qp_b(int kind, const BRefs &b);
    bool p2_load(const char *path);
    bool p2_init();
    double p2_pick_qscale(int frame) const;
};

// the float quantiser as the device takes it: beside its rounding (a quantiser clipped into 1..51 from outside has no fraction to carry: 0 = the integer one)
inline float near_qpm(double qpf, int qp) { const float f = (float)qpf; return f > (float)qp - 1.f && f < (float)qp + 1.f ? f : 0.f; }

}  // namespace x264host

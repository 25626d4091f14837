// ratecontrol.cpp — the session's rate control (host/ratecontrol.hpp).
#include "ratecontrol.hpp"
#include <cmath>
#include <stdlib.h>
#include <string>

namespace x264host {

// [x264-upstream] encoder/ratecontrol.c qp2qscale / qscale2qp: single floats (powf / log2f), as x264 has them
static double qp2qscale(double qp) { return (double)(0.85f * powf(2.0f, ((float)qp - 12.0f) / 6.0f)); }
static double qscale2qp(double qscale) { return (double)(12.0f + 6.0f * log2f((float)qscale / 0.85f)); }
static double FL(double v) { return (double)(float)v; }          // an assignment to one of x264's float variables
static double clampd(double v, double lo, double hi) { return v < lo ? lo : v > hi ? hi : v; }
// fdec->f_qp_avg_rc as x264 arrives at it: rc->qpa_rc (a float) gathers qpm * mb_width row by row (x264_ratecontrol_mb), x264_ratecontrol_end divides by the macroblock count
static double qp_avg_rc(float qpm, int mbw, int mbh) { float a = 0.f; for (int y = 0; y < mbh; y++) a += qpm * mbw; return (double)(a / (float)(mbw * mbh)); }

// get_zone: the LAST zone that holds the picture (display index) wins
const RateControl::Zone *RateControl::get_zone(int frame) const
{
    for (size_t i = zones.size(); i-- > 0;) if (frame >= zones[i].start && frame <= zones[i].end) return &zones[i];
    return nullptr;
}
// parse_zones / parse_zone: "<start>,<end>,q=<int>" or "<start>,<end>,b=<float>", zones separated by '/'.  (x264 also lets a zone carry other options after
// the first; those reconfigure the encoder for the zone's pictures and are not implemented: said in the log, the zone keeps its quantiser part)
void RateControl::parse_zones(const x264_param_t &param)
{
    const char *str = param.rc.psz_zones;
    if (!str || !*str) return;
    std::string all(str);
    size_t pos = 0;
    while (pos <= all.size()) {
        const size_t e = all.find('/', pos);
        const std::string z = all.substr(pos, e == std::string::npos ? std::string::npos : e - pos);
        pos = e == std::string::npos ? all.size() + 1 : e + 1;
        if (z.empty()) continue;
        Zone zn = { 0, 0, false, 0, 1.f };
        int len = 0;
        if (sscanf(z.c_str(), "%d,%d,q=%d%n", &zn.start, &zn.end, &zn.qp, &len) >= 3) zn.force_qp = true;
        else if (sscanf(z.c_str(), "%d,%d,b=%f%n", &zn.start, &zn.end, &zn.bitrate_factor, &len) >= 3) zn.force_qp = false;
        else if (sscanf(z.c_str(), "%d,%d%n", &zn.start, &zn.end, &len) >= 2) zn.bitrate_factor = 1.f;
        else { xlog(&param, X264_LOG_ERROR, "invalid zone: \"%s\"\n", z.c_str()); continue; }
        if (zn.start > zn.end) { xlog(&param, X264_LOG_ERROR, "invalid zone: start=%d end=%d\n", zn.start, zn.end); continue; }
        if (!zn.force_qp && zn.bitrate_factor <= 0) { xlog(&param, X264_LOG_ERROR, "invalid zone: bitrate_factor=%f\n", zn.bitrate_factor); continue; }
        if ((size_t)len < z.size()) xlog(&param, X264_LOG_WARNING, "zone %d,%d: per-zone encoder options (\"%s\") are not implemented in the MI355X path: the zone keeps its quantiser / bitrate part only\n", zn.start, zn.end, z.c_str() + len);
        zones.push_back(zn);
    }
}

bool RateControl::open(const x264_param_t &param, int mbw_, int mbh_, int bframes, int qp_i, int qp_p)
{
    p = &param;
    mbw = mbw_; mbh = mbh_; nmb = mbw * mbh;
    mbtree = p->rc.b_mb_tree != 0 || tree_read;
    // x264_ratecontrol_init_reconfigurable: ip_offset = 6.0 * log2f( f_ip_factor ), pb_offset = 6.0 * log2f( f_pb_factor )
    ip_factor = fabs(p->rc.f_ip_factor) > 0 ? fabs(p->rc.f_ip_factor) : 1.0; pb_factor = fabs(p->rc.f_pb_factor) > 0 ? fabs(p->rc.f_pb_factor) : 1.0;
    ip_offset = 6.0 * log2f((float)ip_factor); pb_offset = 6.0 * log2f((float)pb_factor);
    lmin = qp2qscale(p->rc.i_qp_min); lmax = qp2qscale(p->rc.i_qp_max);
    fps = p->i_fps_num ? (double)p->i_fps_num / p->i_fps_den : 25.0;          // (every session: the second pass reads it too)
    // constant quantisers by picture type: B from P by --pbratio, a B-reference halfway between them
    const int qp_b = clampi((int)(qp_p + pb_offset + 0.5), 0, 51);
    qp_constant[PIC_IDR] = qp_constant[PIC_I] = qp_i; qp_constant[PIC_P] = qp_p; qp_constant[PIC_BREF] = (qp_b + qp_p) / 2; qp_constant[PIC_B] = qp_b;
    if (by_cost()) {
        // x264_ratecontrol_new: rate_factor_constant = base_cplx^(1 - qcomp) / qp2qscale(crf), base_cplx = mbs * (bframes ? 120 : 80)
        qcompress = p->rc.f_qcompress;
        if (mbtree) qcompress = 1.0;                     // the tree does the complexity weighting, CRF shifts by 13.5 (1 - qcomp)
        rate_factor_constant = pow((double)nmb * (bframes ? 120.0 : 80.0), 1.0 - qcompress) / qp2qscale(p->rc.f_rf_constant + (mbtree ? (1.0 - p->rc.f_qcompress) * 13.5 : 0.0));
        // (b_abr = CRF and ABR alike): the running P quantiser starts with a hundredth of a picture at ABR_INIT_QP (CRF: the rate factor; ABR: 24)
        const double abr_init_qp = crf ? (double)p->rc.f_rf_constant : 24.0;
        accum_p_norm = .01; accum_p_qp = abr_init_qp * accum_p_norm;
        last_qscale_for[0] = last_qscale_for[1] = qp2qscale(abr_init_qp);
        dur_ratio = clampd(p->i_fps_num ? (double)p->i_fps_den / p->i_fps_num : 0.04, 0.01, 1.0) / 0.04;          // CLIP_DURATION / BASE_FRAME_DURATION
    }
    if (abr) {
        // x264_ratecontrol_new / x264_ratecontrol_init_reconfigurable, ABR without VBV
        bitrate = p->rc.i_bitrate * 1000.0;
        cplxr_sum = 0.01 * pow(7.0e5, qcompress) * pow((double)nmb, 0.5);
        wanted_bits_window = bitrate / fps;
        abr_buffer = 2.0 * (p->rc.f_rate_tolerance > 0.01f ? p->rc.f_rate_tolerance : 0.01f) * bitrate;
        lstep = pow(2.0, (p->rc.i_qp_step > 0 ? p->rc.i_qp_step : 4) / 6.0);
    }
    if (vbv) {
        // x264_ratecontrol_init_reconfigurable with the parameters x264_encoder_open validated (kbit -> bit; the HRD, when signalled, carries these unscaled values)
        vbv_max_rate = hrd_rate ? hrd_rate : p->rc.i_vbv_max_bitrate * 1000.0; buffer_size = hrd_size ? hrd_size : p->rc.i_vbv_buffer_size * 1000.0;
        buffer_rate = vbv_max_rate / fps;
        single_frame_vbv = buffer_rate * 1.1 > buffer_size;
        vbv_min_rate = abr && p->rc.i_vbv_max_bitrate <= p->rc.i_bitrate;
        cbr_decay = 1.0;
        if (abr) { const double t = 1.5 - buffer_rate * fps / bitrate; cbr_decay = 1.0 - buffer_rate / buffer_size * 0.5 * (t > 0 ? t : 0); }
        buffer_fill_final = buffer_size * p->rc.f_vbv_buffer_init;
        // x264_ratecontrol_new: the size predictors by slice type (coefficients 1.0 / 1.0 / 1.5 for P / B / I), and a B picture's size from the P picture behind it
        const float coeff[3] = { 1.5f, 1.0f, 1.0f };
        for (int i = 0; i < 3; i++) pred[i] = { coeff[i] / 2, coeff[i], 1.0f, 0.5f, 0.0f };
        pred_b_from_p = { 0.5f / 2, 0.5f, 1.0f, 0.5f, 0.0f };
        level_mbps = 0; level_mincr = 2;
        for (int i = 0; x264_levels[i].level_idc; i++) if (x264_levels[i].level_idc == p->i_level_idc) { level_mbps = x264_levels[i].mbps; level_mincr = x264_levels[i].mincr; }
    }
    if (pass2 && mbtree) {          // as single-pass tree sessions have them (pb_factor stays the session's there, and here)
        qcompress = 1.0;
        dur_ratio = clampd(p->i_fps_num ? (double)p->i_fps_den / p->i_fps_num : 0.04, 0.01, 1.0) / 0.04;
    }
    if (pass2) {
        if (!p2_load(p->rc.psz_stat_in) || !p2_init()) return false;
        xlog(p, X264_LOG_INFO, "2-pass: %d pictures planned from the first pass' statistics, %.1f kbit expected before the last one\n", (int)p2.size(), p2_final_bits / 1000.0);
    }
    // (the driver's N-th pass asks for both, statistics read AND written again — codec.c:1519-1541 — so that a further pass plans from this one's pictures)
    const bool stat_update = pass2 && p->rc.b_stat_write && p->rc.psz_stat_out;
    if (pass1 || stat_update) {
        // x264 writes <stats>.temp and renames it when the encoder closes; the first line names the options the second pass must agree with
        stat_file = fopen((std::string(p->rc.psz_stat_out) + ".temp").c_str(), "wb");
        if (!stat_file) { xlog(p, X264_LOG_ERROR, "ratecontrol_init: can't open stats file\n"); return false; }
        fprintf(stat_file, "#options: %dx%d fps=%u/%u timebase=%u/%u bitdepth=8 cabac=%d ref=%d bframes=%d b_pyramid=%d b_adapt=%d weightp=%d keyint=%d rc=%s", p->i_width, p->i_height,
                p->i_fps_num, p->i_fps_den, p->i_fps_den, p->i_fps_num, p->b_cabac, p->i_frame_reference, p->i_bframe, p->i_bframe_pyramid, p->i_bframe_adaptive,
                p->analyse.i_weighted_pred, p->i_keyint_max, p->rc.i_rc_method == X264_RC_ABR ? "abr" : p->rc.i_rc_method == X264_RC_CRF ? "crf" : "cqp");
        if (tree_write && pass1) fprintf(stat_file, " mbtree=1 rc_lookahead=%d", p->rc.i_lookahead);          // a first pass that writes <stats>.mbtree beside them
        fprintf(stat_file, "\n");
    }
    return true;
}

// rate_estimate_qscale for an I or P picture (single-pass CRF / ABR): a function of the lookahead costs, the picture type and the running state only (ABR adds the
// coded sizes through end()), so under CRF it can run when a picture ARRIVES — which is what lets GOP-parallel sessions keep CRF's quantisers
double RateControl::pick_qp(bool is_i, const int32_t costs[4], int frame)
{
    // q = rceq / rate_factor; rceq = blurred_complexity^(1 - qcomp), or under macroblock-tree (which weights the complexity itself) the frame-duration term alone
    const double satd = is_i ? costs[0] : costs[1];
    cplxsum = cplxsum * 0.5 + satd / dur_ratio;
    cplxcount = cplxcount * 0.5 + 1.0;
    double q, overflow = 1.0;
    const double rate_factor = crf ? rate_factor_constant : wanted_bits_window / cplxr_sum;
    if (satd > 0) {
        last_rceq = mbtree ? pow(1.0 / dur_ratio, 1.0 - p->rc.f_qcompress) : pow(cplxsum / cplxcount, 1.0 - qcompress);
        q = FL(last_rceq / rate_factor);          // (rate_estimate_qscale's q is a float: every assignment rounds)
    } else q = FL(last_qscale_for[is_i ? 0 : 1]);
    // get_qscale: a zone forces its quantiser or scales the picture's bits (an I picture after P pictures still takes the running P quantiser below, as in x264)
    if (const Zone *z = get_zone(frame)) q = FL(z->force_qp ? qp2qscale(z->qp) : q / z->bitrate_factor);
    last_satd = satd;
    if (abr && satd > 0 && !vbv_min_rate) {
        // pull towards the target: bits so far against time so far, within an abr_buffer that grows with sqrt(time)
        const double time_done = frames_done / fps, wanted_bits = time_done * bitrate;
        if (wanted_bits > 0) {
            const double buf = abr_buffer * (time_done > 1.0 ? sqrt(time_done) : 1.0);
            overflow = clampd(1.0 + (total_bits - wanted_bits) / buf, 0.5, 2.0);
            q = FL(q * overflow);
        }
    }
    if (is_i && p->i_keyint_max > 1 && !last_non_b_is_i) q = FL(qp2qscale(accum_p_qp / accum_p_norm) / ip_factor);
    else if (frames_done > 0) {
        if (abr) {       // asymmetric clipping against the last quantiser of the same picture type (qpstep)
            double lo = last_qscale_for[is_i ? 0 : 1] / lstep, hi = last_qscale_for[is_i ? 0 : 1] * lstep;
            if (overflow > 1.1 && frames_done > 3) hi *= lstep;
            else if (overflow < 0.9) lo /= lstep;
            q = FL(clampd(q, lo, hi));
        }
    } else if (crf && qcompress != 1.0) q = FL(qp2qscale(p->rc.f_rf_constant) / ip_factor);       // very first picture: ABR_INIT_QP / ipratio
    if (vbv) {
        qp_novbv = qscale2qp(q);
        q = FL(clip_qscale(is_i, q));
    } else
    q = FL(clampd(q, lmin, lmax));
    last_qscale_for[is_i ? 0 : 1] = q;
    if (frames_done == 0) last_qscale_for[1] = q * ip_factor;
    if (vbv) {
        // rate_estimate_qscale: the size the picture is expected to take (a single-frame buffer is always used up), limited by MinCR
        frame_size_planned = single_frame_vbv ? buffer_rate : predict_size(pred[is_i ? 0 : 1], q, last_satd);
        if (frame_size_planned > frame_size_maximum) frame_size_planned = frame_size_maximum;
    }
    const double qpf = clampd(qscale2qp(q), p->rc.i_qp_min, p->rc.i_qp_max);
    accum_p_qp = accum_p_qp * 0.95 + (is_i ? qpf + ip_offset : qpf);      // accum_p_qp_update
    accum_p_norm = accum_p_norm * 0.95 + 1.0;
    last_non_b_is_i = is_i;
    return qpf;
}

// rate_estimate_qscale's B branch in x264's own types: float q0, q1, q (f_qp_avg_rc of the nearest references), double offsets; the result goes through qp2qscale
// and x264_ratecontrol_start's qscale2qp like every quantiser
double RateControl::pick_qp_b(int kind, const BRefs &b)
{
    const int s0 = b.slot[0], s1 = b.slot[1], dt0 = b.dpoc[0], dt1 = b.dpoc[1];
    const bool i0 = slot_kind[s0] == PIC_IDR || slot_kind[s0] == PIC_I, i1 = slot_kind[s1] == PIC_IDR || slot_kind[s1] == PIC_I;
    float q0 = (float)slot_qp_rc[s0], q1 = (float)slot_qp_rc[s1], qf;
    if (slot_kind[s0] == PIC_BREF) q0 = (float)(q0 - pb_offset / 2);
    if (slot_kind[s1] == PIC_BREF) q1 = (float)(q1 - pb_offset / 2);
    if (i0 && i1) qf = (float)((q0 + q1) / 2 + ip_offset);
    else if (i0) qf = q1;
    else if (i1) qf = q0;
    else qf = (q0 * dt1 + q1 * dt0) / (dt0 + dt1);
    qf = (float)(qf + (kind == PIC_BREF ? pb_offset / 2 : pb_offset));
    const double q = clampd(qscale2qp(qp2qscale(qf)), p->rc.i_qp_min, p->rc.i_qp_max);
    if (vbv) {
        // B pictures are not clipped (the P pictures' quantisers control them); their cost is the list-1 reference's, their planned size the B predictor's of it
        last_satd = slot_satd[s1];
        qp_novbv = qf;
        frame_size_planned = predict_size(pred[2], qp2qscale(qf), last_satd);
        if (frame_size_planned > frame_size_maximum) frame_size_planned = frame_size_maximum;
    }
    // x264_ratecontrol_start: accum_p_qp_update runs for every picture type — a B picture's own quantiser (no ip_offset) enters the running average an I picture
    // after P pictures takes its quantiser from
    accum_p_qp = accum_p_qp * 0.95 + q;
    accum_p_norm = accum_p_norm * 0.95 + 1.0;
    return q;
}

int RateControl::start(int kind, int frame, const int32_t costs[4], const BRefs *b, double *qpf)
{
    const bool is_i = kind == PIC_IDR || kind == PIC_I, is_b = kind == PIC_B || kind == PIC_BREF;
    double q; int qp;
    if (vbv) {
        // update_vbv_plan: what the buffer holds when this picture is removed, less the header NAL units already written for it
        buffer_fill = (buffer_fill_final < buffer_size ? buffer_fill_final : buffer_size) - (double)cur_overhead;
        // x264_ratecontrol_start: the largest picture the level allows (Table A-1 MaxMBPS and MinCR; "the spec has a bizarre special case for the first frame")
        if (frames_done == 0) { const double fr = 1.0 / (p->i_level_idc >= 60 ? 300 : 172); frame_size_maximum = 384 * 8 * ((double)nmb > fr * level_mbps ? (double)nmb : fr * level_mbps) / level_mincr; }
        else frame_size_maximum = 384 * 8 * (1.0 / fps) * level_mbps / level_mincr;
    }
    if (pass2) {          // the plan with feedback (zones are not applied to it)
        q = clampd(qscale2qp(p2_pick_qscale(frame)), p->rc.i_qp_min, p->rc.i_qp_max);
        qp = clampi((int)(q + 0.5), 1, 51);
    } else if (!by_cost()) {          // constant quantiser by picture type; a zone shifts it by (its qp - the P quantiser), or by -6 log2f(bitrate factor)
        qp = qp_constant[kind];
        if (const Zone *z = get_zone(frame)) {
            float qf = (float)qp;
            if (z->force_qp) qf += (float)(z->qp - qp_constant[PIC_P]); else qf -= 6.f * log2f(z->bitrate_factor);
            const float lo = (float)p->rc.i_qp_min, hi = (float)(p->rc.i_qp_max < 51 ? p->rc.i_qp_max : 51);
            qp = clampi((int)((qf < lo ? lo : qf > hi ? hi : qf) + 0.5f), 0, 51);
        }
        q = qp;
    } else if (is_b) {          // (the integer quantiser of a B picture is clamped to [qpmin, qpmax], the others' to [1, 51] after the float clamp)
        q = pick_qp_b(kind, *b);
        qp = clampi((int)(q + 0.5), p->rc.i_qp_min, p->rc.i_qp_max);
    } else {
        q = pick_qp(is_i, costs, frame);
        qp = clampi((int)(q + 0.5), 1, 51);
    }
    frames_done++;
    if (qpf) *qpf = q;
    return qp;
}

void RateControl::kept(int slot, double qpf, int kind) { slot_qp_rc[slot] = qp_avg_rc((float)qpf, mbw, mbh); slot_kind[slot] = kind; slot_satd[slot] = last_satd; }

void RateControl::vbv_picture(const Planned *planned, int bframes, bool last_minigop_b, long overhead_bits) { cur_planned = planned; cur_bframes = bframes; cur_last_b = last_minigop_b; cur_overhead = overhead_bits; }
int RateControl::qp_ceiling() const { return p->rc.i_qp_max < 51 ? p->rc.i_qp_max : 51; }

// predict_size / update_predictor: x264's, in its single floats
double RateControl::predict_size(const Predictor &pr, double q, double var) { return (double)((pr.coeff * (float)var + pr.offset) / ((float)q * pr.count)); }
void RateControl::update_predictor(Predictor &pr, double q_, double var_, double bits_)
{
    const float q = (float)q_, var = (float)var_, bits = (float)bits_, range = 1.5f;
    if (var < 10) return;
    const float old_coeff = pr.coeff / pr.count, old_offset = pr.offset / pr.count;
    float new_coeff = (bits * q - old_offset) / var;
    if (new_coeff < pr.coeff_min) new_coeff = pr.coeff_min;
    const float new_coeff_clipped = new_coeff < old_coeff / range ? old_coeff / range : new_coeff > old_coeff * range ? old_coeff * range : new_coeff;
    float new_offset = bits * q - new_coeff_clipped * var;
    if (new_offset >= 0) new_coeff = new_coeff_clipped; else new_offset = 0;
    pr.count *= pr.decay; pr.coeff *= pr.decay; pr.offset *= pr.decay;
    pr.count++; pr.coeff += new_coeff; pr.offset += new_offset;
}

// clip_qscale for an I or P picture (q: double throughout, as in x264; the caller's float takes the result): raise the quantiser until neither this picture nor
// the planned ones behind it under-run the buffer, lower it (only when the rate is a minimum too) while the buffer would end too full
double RateControl::clip_qscale(bool is_i, double q)
{
    const double q0 = q;
    const Predictor &pt = pred[is_i ? 0 : 1];
    if (last_satd > 0) {
        const double dur = 1.0 / fps;          // (constant frame rate: every cpb duration is one picture's)
        if (vbv_lookahead) {
            int terminate = 0;
            for (int it = 0; it < 1000 && terminate != 3; it++) {
                double cur_bits = predict_size(pt, q, last_satd), fill = buffer_fill - cur_bits, total_duration = 0;
                double frame_q[3];          // as pred[]: [0] I, [1] P, [2] B
                frame_q[1] = is_i ? q * p->rc.f_ip_factor : q; frame_q[2] = frame_q[1] * p->rc.f_pb_factor; frame_q[0] = frame_q[1] / p->rc.f_ip_factor;
                for (int j = 0; fill >= 0 && fill <= buffer_size; j++) {
                    total_duration += dur;
                    fill += vbv_max_rate * dur;
                    const int t = cur_planned && j < PLAN_MAX ? cur_planned->type[j] : (int)PLAN_END;
                    if (t == PLAN_END) break;
                    const int k = t == PIC_IDR || t == PIC_I ? 0 : t == PIC_P ? 1 : 2;
                    fill -= predict_size(pred[k], frame_q[k], cur_planned->satd[j]);
                }
                double target = buffer_fill + total_duration * vbv_max_rate * 0.5;          // at least half full, but no impossible goal
                if (target > buffer_size * 0.5) target = buffer_size * 0.5;
                if (fill < target) { q *= 1.01; terminate |= 1; continue; }
                target = clampd(buffer_fill - total_duration * vbv_max_rate * 0.5, buffer_size * 0.8, buffer_size);          // no more than 80 % full
                if (vbv_min_rate && fill > target) { q /= 1.01; terminate |= 2; continue; }
                break;
            }
        } else {
            // the purely reactive algorithm
            if ((!is_i || last_non_b_is_i) && buffer_fill / buffer_size < 0.5) q /= clampd(2.0 * buffer_fill / buffer_size, 0.5, 1.0);
            // a hard threshold so that the picture fits (mostly for I pictures); small buffers may be used up entirely, a single-frame buffer must be
            double bits = predict_size(pt, q, last_satd);
            const double max_fill_factor = p->rc.i_vbv_buffer_size >= 5 * p->rc.i_vbv_max_bitrate / fps ? 2 : 1, min_fill_factor = single_frame_vbv ? 1 : 2;
            if (bits > buffer_fill / max_fill_factor) { const double qf = clampd(buffer_fill / (max_fill_factor * bits), 0.2, 1.0); q /= qf; bits *= qf; }
            if (bits < buffer_rate / min_fill_factor) { const double qf = clampd(bits * min_fill_factor / buffer_rate, 0.001, 1.0); q *= qf; }
            if (q < q0) q = q0;
        }
        // a P picture: use up the bits that would overflow before the next P picture, going by what the B pictures behind it are expected to take
        if (!is_i && !single_frame_vbv) {
            int nb = cur_bframes;
            const double bits = predict_size(pt, q, last_satd), bbits = predict_size(pred_b_from_p, q * p->rc.f_pb_factor, last_satd);
            double pbbits = bits, bdur = nb * dur;
            if (bbits * nb > bdur * vbv_max_rate) { nb = 0; bdur = 0; }
            pbbits += nb * bbits;
            const double space = buffer_fill + (bdur + dur) * vbv_max_rate - buffer_size;
            if (pbbits < space) { const double a = pbbits / space, b = bits / (0.5 * buffer_size); q *= a > b ? a : b; }
            if (q < q0 / 2) q = q0 / 2;
        }
        // MinCR and the buffer's fill
        const double bits = predict_size(pt, q, last_satd);
        double fmax = buffer_fill > 0.001 ? buffer_fill : 0.001;
        if (fmax > frame_size_maximum) fmax = frame_size_maximum;
        if (bits > fmax) q *= bits / fmax;
        if (!vbv_min_rate && q < q0) q = q0;
    }
    if (lmin == lmax) return lmin;
    return clampd(q, lmin, lmax);
}

static double qscale2bits(const RateControl::Pass2Entry &e, double qscale)
{
    if (qscale < 0.1) qscale = 0.1;
    return (e.tex + .1) * pow(e.qscale / qscale, 1.1) + e.mv * pow((e.qscale > 1 ? e.qscale : 1) / (qscale > 1 ? qscale : 1), 0.5) + e.misc;
}

int RateControl::end(size_t bytes, int kind, int frame, double qpf, const PicStats *st)
{
    const long total = (long)bytes * 8;
    int filler_bytes = 0;
    if (stat_file && st) {
        const char t = kind == PIC_IDR ? 'I' : kind == PIC_I ? 'i' : kind == PIC_P ? 'P' : kind == PIC_BREF ? 'B' : 'b';
        fprintf(stat_file, "in:%d out:%ld type:%c dur:%d cpbdur:%d q:%.2f aq:%.2f tex:%ld mv:%ld misc:%ld imb:%ld pmb:%ld smb:%ld d:%c ref:;\n", frame, coded, t, 1, 1, qpf,
                st->aq_mean, st->tex_bits, st->mv_bits, total - st->mv_bits - st->tex_bits, st->imb, st->pmb, st->smb, st->direct);
    }
    if (pass2) {          // the second pass' account of what was spent against the plan
        p2_total_bits += (double)total;
        if (const Pass2Entry *e = plan(frame)) p2_expected_sum += qscale2bits(*e, qp2qscale(qpf));
    }
    if (abr) {
        // what the picture took moves the rate factor of the pictures to come (a B picture's quantiser is an offset of its neighbours': its bits count divided by pbratio)
        const bool is_b = kind == PIC_B || kind == PIC_BREF;
        total_bits += (double)total;
        cplxr_sum += (double)total * qp2qscale(qp_avg_rc((float)qpf, mbw, mbh)) / (last_rceq * (is_b ? pb_factor : 1.0));          // (rc->qpa_rc: the float gathered row by row)
        wanted_bits_window += bitrate / fps;
        if (vbv) { cplxr_sum *= cbr_decay; wanted_bits_window *= cbr_decay; }
    }
    if (vbv) {
        // update_vbv: the predictor of the picture's type learns from its size, then the buffer's account
        const bool is_b = kind == PIC_B || kind == PIC_BREF, is_i = kind == PIC_IDR || kind == PIC_I;
        const double qs = qp2qscale(qp_avg_rc((float)qpf, mbw, mbh));
        if (last_satd >= nmb) update_predictor(pred[is_i ? 0 : is_b ? 2 : 1], qs, last_satd, (double)total);
        if (is_b) {          // x264_ratecontrol_end: a B picture's size from the P picture's cost, learnt from the run's mean at its last picture
            bframe_bits += (double)total;
            if (cur_last_b) { update_predictor(pred_b_from_p, qs, last_satd, bframe_bits / (cur_bframes > 0 ? cur_bframes : 1)); bframe_bits = 0; }
        }
        buffer_fill_final -= (double)total;
        if (buffer_fill_final < 0) { xlog(p, X264_LOG_WARNING, "VBV underflow (frame %d, %.0f bits)\n", frame, buffer_fill_final); buffer_fill_final = 0; }
        buffer_fill_final += buffer_rate;
        if (filler && buffer_fill_final > buffer_size) {
            // --nal-hrd cbr: what arrives beyond the buffer's size has to be sent (a filler NAL unit is never smaller than its overhead)
            const long over = (long)ceil((buffer_fill_final - buffer_size) / 8.0);
            filler_bytes = (int)(over > filler_overhead() ? over : filler_overhead());
            buffer_fill_final -= 8.0 * filler_bytes;
        } else if (buffer_fill_final > buffer_size) buffer_fill_final = buffer_size;
    }
    coded++;
    return filler_bytes;
}

void RateControl::close()
{
    if (!stat_file) return;
    fclose(stat_file); stat_file = nullptr;
    const std::string out = p->rc.psz_stat_out ? p->rc.psz_stat_out : "";
    if (pass2 && coded < (long)p2.size()) { remove((out + ".temp").c_str()); xlog(p, X264_LOG_INFO, "2-pass: %ld of %d pictures coded: the statistics file keeps the first pass' lines\n", coded, (int)p2.size()); }
    else if (!out.empty() && rename((out + ".temp").c_str(), out.c_str())) xlog(p, X264_LOG_ERROR, "failed to rename \"%s.temp\" to \"%s\"\n", out.c_str(), out.c_str());
}

// ---- 2-pass (x264_ratecontrol_new's statistics parser, init_pass2, get_qscale / get_diff_limited_q, qscale2bits; no VBV, no zones.  The tree is off in these
//      sessions unless the macroblock-tree statistics file is switched on and usable: tree_read, host/mbtreestats.hpp) ----
bool RateControl::p2_load(const char *path)
{
    FILE *f = fopen(path, "rb");
    if (!f) { xlog(p, X264_LOG_ERROR, "ratecontrol_init: can't open stats file\n"); return false; }
    char line[2048];
    std::vector<Pass2Entry> raw;
    while (fgets(line, sizeof(line), f)) {
        if (line[0] == '#') continue;
        Pass2Entry e;
        long long dur = 0, cpbdur = 0;
        float q = 0, aq = 0;
        int tex = 0, mv = 0, misc = 0, imb = 0, pmb = 0, smb = 0;
        char d = '-';
        if (sscanf(line, " in:%d out:%d type:%c dur:%lld cpbdur:%lld q:%f aq:%f tex:%d mv:%d misc:%d imb:%d pmb:%d smb:%d d:%c", &e.in, &e.out, &e.type, &dur, &cpbdur, &q, &aq,
                   &tex, &mv, &misc, &imb, &pmb, &smb, &d) < 13) { fclose(f); xlog(p, X264_LOG_ERROR, "statistics are damaged at line %d, parser out\n", (int)raw.size() + 1); return false; }
        e.qscale = qp2qscale(q); e.tex = tex; e.mv = mv; e.misc = misc; e.icount = imb; e.dur = dur > 0 ? (double)dur : 1.0; e.kept_as_ref = e.type != 'b';
        raw.push_back(e);
    }
    fclose(f);
    if (raw.empty()) { xlog(p, X264_LOG_ERROR, "empty stats file\n"); return false; }
    p2.assign(raw.size(), Pass2Entry()); p2_out.assign(raw.size(), 0);
    for (const auto &e : raw) {
        if (e.in < 0 || e.in >= (int)raw.size() || e.out < 0 || e.out >= (int)raw.size()) { xlog(p, X264_LOG_ERROR, "bad frame number (%d) at stats line\n", e.in); return false; }
        p2[(size_t)e.in] = e; p2_out[(size_t)e.out] = e.in;
    }
    return true;
}
// x264's slice type of a statistics character as the rate control groups them: 0 I, 1 P, 2 B
static int p2_kind(char t) { return t == 'I' || t == 'i' ? 0 : t == 'P' ? 1 : 2; }
bool RateControl::p2_init()
{
    std::vector<Pass2Entry> &E = p2;
    const int n = (int)E.size();
    double duration = 0;
    for (auto &e : E) duration += e.dur;
    duration /= fps * E[0].dur;                               // (durations are in ticks of one picture here: constant frame rate, codec.c:1476-1480)
    const double all_available_bits = p->rc.i_bitrate * 1000.0 * duration;
    // (under the macroblock-tree statistics file rc->qcompress is 1, as in single-pass tree sessions: the tree has done the complexity weighting)
    const double qblur = p->rc.f_qblur, cplxblur = p->rc.f_complexity_blur, qcomp = tree_read ? qcompress : p->rc.f_qcompress;
    const int filter_size = (int)(qblur * 4) | 1;
    const double base_cplx = (double)nmb * (p->i_bframe ? 120 : 80);
    const double qstep = pow(2.0, p->rc.i_qp_step / 6.0);
    double all_const_bits = 0;
    for (auto &e : E) all_const_bits += e.misc;
    if (all_available_bits < all_const_bits) {
        xlog(p, X264_LOG_ERROR, "requested bitrate is too low. estimated minimum is %d kbps\n", (int)(all_const_bits * fps / (n * 1000.)));
        return false;
    }
    // blur the complexities (not the quantisers: one very simple picture must not drag its neighbours down); per unit of BASE_FRAME_DURATION as x264 has it
    const double frame_duration = clampd(1.0 / fps, 0.01, 1.0) / 0.04;
    for (int i = 0; i < n; i++) {
        double weight_sum = 0, cplx_sum = 0, weight = 1.0;
        for (int j = 1; j < cplxblur * 2 && j < n - i; j++) {
            const auto &r = E[(size_t)(i + j)];
            weight *= 1 - pow((float)r.icount / (float)nmb, 2);          // (x264: a float division — i_count and nmb are integers there)
            if (weight < .0001) break;
            const double g = weight * exp(-j * j / 200.0);
            weight_sum += g; cplx_sum += g * (qscale2bits(r, 1) - r.misc) / frame_duration;
        }
        weight = 1.0;
        for (int j = 0; j <= cplxblur * 2 && j <= i; j++) {
            const auto &r = E[(size_t)(i - j)];
            const double g = weight * exp(-j * j / 200.0);
            weight_sum += g; cplx_sum += g * (qscale2bits(r, 1) - r.misc) / frame_duration;
            weight *= 1 - pow((float)r.icount / (float)nmb, 2);          // (x264: a float division — i_count and nmb are integers there)
            if (weight < .0001) break;
        }
        E[(size_t)i].blurred = FL(cplx_sum / weight_sum);          // (ratecontrol_entry_t keeps blurred_complexity as a float)
    }
    // the rate factor: multiplied into every picture's RCEQ value it makes the sizes add up to the request (no closed form: qscale2bits does not invert)
    std::vector<double> qscale((size_t)n), blurred((size_t)n);
    double last_q[3], acc_p_qp = 0, acc_p_norm = 0, last_acc_p_norm = 1;
    int last_non_b = -1;
    auto get_qscale = [&](const Pass2Entry &e, double rate_factor) {
        // the RCEQ value; under the tree the frame-duration term alone (pick_qp's expression for single-pass tree sessions)
        double q = tree_read ? pow(1.0 / dur_ratio, 1.0 - p->rc.f_qcompress) : pow(e.blurred, 1 - qcomp);
        if (!std::isfinite(q) || e.tex + e.mv == 0) q = last_q[p2_kind(e.type)];
        else q /= rate_factor;
        return q;
    };
    auto diff_limited = [&](const Pass2Entry &e, double q) {
        const int kind = p2_kind(e.type);
        const double last_p_q = last_q[1], last_non_b_q = last_non_b >= 0 ? last_q[last_non_b] : q;
        if (kind == 0) {
            const double iq = q, pq = acc_p_norm > 0 ? qp2qscale(acc_p_qp / acc_p_norm) : q;
            if (acc_p_norm <= 0) q = iq;
            else if (p->rc.f_ip_factor < 0) q = iq / ip_factor;
            else if (acc_p_norm >= 1) q = pq / ip_factor;
            else q = acc_p_norm * pq / ip_factor + (1 - acc_p_norm) * iq;
        } else if (kind == 2) {
            if (p->rc.f_pb_factor > 0) q = last_non_b_q;
            if (!e.kept_as_ref) q *= pb_factor;
        } else if (last_non_b == 1 && e.tex == 0) q = last_p_q;
        if (last_non_b == kind && (kind != 0 || last_acc_p_norm < 1)) {
            const double lq = last_q[kind];
            q = clampd(q, lq / qstep, lq * qstep);
        }
        last_q[kind] = q;
        if (kind != 2) last_non_b = kind;
        if (kind == 0) { last_acc_p_norm = acc_p_norm; acc_p_norm = 0; acc_p_qp = 0; }
        if (kind == 1) { const float mask = (float)(1 - pow((float)e.icount / (float)nmb, 2)); acc_p_qp          /* (a float in x264) */ = mask * (qscale2qp(q) + acc_p_qp); acc_p_norm = mask * (1 + acc_p_norm); }
        return q;
    };
    double expected_bits = 1;
    last_q[0] = last_q[1] = last_q[2] = pow(base_cplx, 1 - qcomp);
    for (int i = 0; i < n; i++) { const double q = get_qscale(E[(size_t)i], 1.0); expected_bits += qscale2bits(E[(size_t)i], q); last_q[p2_kind(E[(size_t)i].type)] = q; }
    const double step_mult = all_available_bits / expected_bits;
    double rate_factor = 0;
    for (double step = 1E4 * step_mult; step > 1E-7 * step_mult; step *= 0.5) {
        expected_bits = 0;
        rate_factor += step;
        last_non_b = -1; last_acc_p_norm = 1; acc_p_norm = 0; acc_p_qp = 0;
        last_q[0] = last_q[1] = last_q[2] = pow(base_cplx, 1 - qcomp) / rate_factor;
        for (int i = 0; i < n; i++) { qscale[(size_t)i] = get_qscale(E[(size_t)i], rate_factor); last_q[p2_kind(E[(size_t)i].type)] = qscale[(size_t)i]; }
        for (int i = n - 1; i >= 0; i--) qscale[(size_t)i] = diff_limited(E[(size_t)i], qscale[(size_t)i]);       // fixed I / B quantisers relative to P
        if (filter_size > 1) {                                  // smooth the curve over pictures of the same kind
            for (int i = 0; i < n; i++) {
                double q = 0.0, sum = 0.0;
                for (int j = 0; j < filter_size; j++) {
                    const int idx = i + j - filter_size / 2;
                    const double d = idx - i, coeff = qblur == 0 ? 1.0 : exp(-d * d / (qblur * qblur));
                    if (idx < 0 || idx >= n) continue;
                    if (p2_kind(E[(size_t)i].type) != p2_kind(E[(size_t)idx].type)) continue;
                    q += qscale[(size_t)idx] * coeff; sum += coeff;
                }
                blurred[(size_t)i] = q / sum;
            }
        } else blurred = qscale;
        for (int i = 0; i < n; i++) {
            const double q = clampd(blurred[(size_t)i], lmin, lmax);          // clip_qscale without VBV
            E[(size_t)i].new_qscale = q;
            expected_bits += qscale2bits(E[(size_t)i], q);
        }
        if (expected_bits > all_available_bits) rate_factor -= step;
    }
    // the plan in coding order: what should have been spent when each picture starts
    expected_bits = 0;
    for (int k = 0; k < n; k++) { auto &e = E[(size_t)p2_out[(size_t)k]]; e.expected_bits = expected_bits; expected_bits += qscale2bits(e, e.new_qscale); }
    p2_final_bits = n > 0 ? E[(size_t)p2_out[(size_t)(n - 1)]].expected_bits : 0;          // x264: entry_out[num_entries - 1]->expected_bits — what should have been spent BEFORE the last picture
    if (fabs(expected_bits / all_available_bits - 1.0) > 0.01) {
        double avgq = 0;
        for (auto &e : E) avgq += e.new_qscale;
        avgq = qscale2qp(avgq / n);
        xlog(p, X264_LOG_WARNING, "Error: 2pass curve failed to converge\n");
        xlog(p, X264_LOG_WARNING, "target: %.2f kbit/s, expected: %.2f kbit/s, avg QP: %.4f\n", (double)p->rc.i_bitrate, expected_bits / duration / 1000., avgq);
    }
    p2_abr_buffer = 2 * p->rc.f_rate_tolerance * p->rc.i_bitrate * 1000.0;
    return true;
}
// rate_estimate_qscale, 2-pass branch: the planned quantiser of display picture `frame`, pulled by how far the coded size is from the plan
// (a second pass codes one picture at a time: `coded`, the pictures that have ended, is x264's h->i_frame)
double RateControl::p2_pick_qscale(int frame) const
{
    const int n = (int)p2.size();
    if (frame >= n) return p2[(size_t)(n - 1)].new_qscale;           // (x264: "2nd pass has more frames than 1st pass", then constant quantiser)
    const Pass2Entry &e = p2[(size_t)frame];
    double buffer = p2_abr_buffer;
    if (n > coded) {           // adjust the buffer by the distance to the end of the video
        const double video_pos = p2_final_bits > 0 ? e.expected_bits / p2_final_bits : 1.0, scale_factor = sqrt((1 - video_pos) * n);
        buffer *= 0.5 * (scale_factor > 0.5 ? scale_factor : 0.5);
    }
    const double diff = (double)((long long)p2_total_bits - (long long)e.expected_bits);          // (x264: int64_t diff = predicted_bits - (int64_t)rce.expected_bits)
    double q = e.new_qscale;
    q /= clampd((buffer - diff) / buffer, .5, 2);
    if (coded >= fps && p2_expected_sum >= 1) {          // x264: h->i_frame >= rcc->fps && rcc->expected_bits_sum >= 1
        const double cur_time = (double)coded / n;
        q *= pow(p2_total_bits / p2_expected_sum, clampd(cur_time * 100, 0, 1));
    }
    return clampd(q, lmin, lmax);
}

}  // namespace x264host

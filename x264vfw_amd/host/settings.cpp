// settings.cpp — x264_encoder_open's rules, step by step (host/settings.hpp).  Each step logs what it changes; the steps depend on their order, which settle() fixes.
#include "settings.hpp"
#include "gopslots.hpp"
#include "noisereduction.hpp"
#include <limits.h>
#include <math.h>
#include <stdlib.h>
#include <thread>

namespace x264host {

static int pick_level(const x264_param_t *p, int mbs, int refs)
{
    double fps = p->i_fps_den ? (double)p->i_fps_num / p->i_fps_den : 25.0;
    for (int i = 0; x264_levels[i].level_idc; i++) {
        const x264_level_t &l = x264_levels[i];
        if (l.level_idc == 9) continue;
        if (l.frame_size >= mbs && l.mbps >= (int)(mbs * fps) && l.dpb >= mbs * refs) return l.level_idc;
    }
    return 62;
}

static int psy_trellis_q8(const x264_param_t &p) { return p.analyse.i_trellis ? (int)(p.analyse.f_psy_trellis / 4 * 256 + 0.5f) : 0; }      // h->mb.i_psy_trellis
static int psy_rd_q8(const x264_param_t &p) { return p.analyse.i_subpel_refine >= 6 ? (int)(p.analyse.f_psy_rd * 256.0f + 0.5f) : 0; }      // h->mb.i_psy_rd

void Settings::settle(x264_param_t &p, RateControl &rc, Dpb &dpb, MbTreeStats &tstats, int &batch_want)
{
    if (const char *e = getenv("X264GPU_BATCH")) { env.batch_set = true; env.batch = atoi(e); }
    if (const char *e = getenv("X264GPU_GOP_SLOTS")) env.gop_slots = atoi(e);
    if (const char *e = getenv("X264GPU_GOP_SLOTS_RC")) env.gop_slots_rc = atoi(e) == 1;
    if (const char *e = getenv("X264GPU_INFLIGHT")) { env.inflight_set = true; env.inflight = atoi(e); }
    env.dump_records = getenv("X264GPU_DUMP_RECORDS") != nullptr;
    if (const char *e = getenv("X264GPU_HOST_PIPELINE")) env.pipeline_off = e[0] == '0';
    if (const char *e = getenv("X264GPU_CAVLC_THREADS")) { env.cavlc_threads_set = true; env.cavlc_threads = atoi(e); }
    env.mbtree_stats = MbTreeStats::opted_in();
    if (const char *e = getenv("X264GPU_QP_RD")) env.qp_rd = atoi(e) == 1;
    if (const char *e = getenv("X264GPU_NR_ANY")) env.nr_any = atoi(e) == 1;

    mbw = (p.i_width + 15) / 16; mbh = (p.i_height + 15) / 16; nmb = mbw * mbh;
    if (!p.i_timebase_num || !p.i_timebase_den) { p.i_timebase_num = p.i_fps_den; p.i_timebase_den = p.i_fps_num; }
    toolset(p);
    // GOP slots with quantisers planned ahead (opt-in): CRF with B pictures under --threads G, nothing that reads coded sizes or shares the session's state
    // (decided on what was asked for; in_flight() withdraws it when the slots do not fit)
    slots_rc = env.gop_slots_rc && p.i_threads > 1 && p.rc.i_rc_method == X264_RC_CRF && p.rc.f_rf_constant >= 1.0f && p.i_bframe > 0 && p.i_keyint_max >= 2 &&
               p.i_keyint_max < (1 << 20) && p.rc.i_vbv_max_bitrate <= 0 && p.rc.i_vbv_buffer_size <= 0 && !p.rc.b_stat_read && !p.rc.b_stat_write && env.batch < 2 &&
               !p.analyse.i_noise_reduction;
    vbv_rules(p);
    modes(p, batch_want);
    quantisers(p, rc, dpb, tstats);
    in_flight(p, rc, dpb, batch_want);
    lookahead_window(p, rc, tstats);
    { const unsigned hw = std::thread::hardware_concurrency();
      cavlc_threads = G > 1 ? 1 : clampi(env.cavlc_threads_set ? env.cavlc_threads : hw >= 32 ? 16 : hw >= 16 ? 8 : hw >= 4 ? (int)hw / 2 : 1, 1, 64); }
}

// the toolset: what this pipeline implements of the analysis options, slices and threads (reported back via x264_encoder_parameters)
void Settings::toolset(x264_param_t &p)
{
    // B pictures: on the device in CABAC sessions, one GOP in flight (settled in modes(), once those are known)
    p.i_bframe = clampi(p.i_bframe, 0, 16);
    if (p.i_frame_reference > 5) { xlog(&p, X264_LOG_INFO, "ref %d -> 5 (DPB of the MI355X path holds up to 5 references)\n", p.i_frame_reference); p.i_frame_reference = 5; }
    if (p.i_frame_reference < 1) p.i_frame_reference = 1;
    p.analyse.b_mixed_references = p.analyse.b_mixed_references && p.i_frame_reference > 1;      // x264 validate_parameters
    p.b_cabac = p.b_cabac != 0;
    if (p.b_cabac && p.i_cabac_init_idc != 0) { xlog(&p, X264_LOG_WARNING, "cabac-idc %d: only the context tables of cabac_init_idc 0 (x264's default) are in the MI355X path: cabac-idc 0\n", p.i_cabac_init_idc); p.i_cabac_init_idc = 0; }
    // --weightp: settled in modes() with the B-picture settings (2 = x264's blind duplicate of reference 0 in sessions that run on the DPB model;
    // the fade analysis that produces other weights — x264_weights_analyse, all that --weightp 1 does — is not implemented)
    p.analyse.i_weighted_pred = clampi(p.analyse.i_weighted_pred, X264_WEIGHTP_NONE, X264_WEIGHTP_SMART); p.analyse.b_weighted_bipred = p.analyse.b_weighted_bipred != 0;
    p.analyse.b_transform_8x8 = p.analyse.b_transform_8x8 != 0;
    if (p.analyse.inter & X264_ANALYSE_PSUB8x8) xlog(&p, X264_LOG_WARNING, "partitions p4x4 (8x4 / 4x8 / 4x4 searches inside P_8x8) are not implemented in the MI355X path: p8x8 stays, p4x4 off\n");
    p.analyse.inter &= X264_ANALYSE_I4x4 | X264_ANALYSE_I8x8 | X264_ANALYSE_PSUB16x16 | X264_ANALYSE_BSUB16x16; p.analyse.intra &= X264_ANALYSE_I4x4 | X264_ANALYSE_I8x8;
    if (!p.analyse.b_transform_8x8) { p.analyse.inter &= ~X264_ANALYSE_I8x8; p.analyse.intra &= ~X264_ANALYSE_I8x8; }   // as x264 validate_parameters
    p.analyse.i_trellis = clampi(p.analyse.i_trellis, 0, 2);          // settled below, once the sub-pel level is known
    p.i_scenecut_threshold = clampi(p.i_scenecut_threshold, 0, 100);
    if (p.analyse.i_me_method > X264_ME_ESA) { xlog(&p, X264_LOG_WARNING, "me tesa is not implemented in the MI355X path yet: me esa\n"); p.analyse.i_me_method = X264_ME_ESA; }
    p.analyse.i_me_range = clampi(p.analyse.i_me_range, 4, p.analyse.i_me_method == X264_ME_UMH ? 64 : 16);     // x264 caps dia/hex at 16; esa: the LDS search window
    // subme 6 / 7 = RD mode decision in P and I slices (x264's i_mbrd 1): on the device, with the bit counts of the session's entropy coder
    // (CAVLC: exact; CABAC: x264's size-only coder on the slice's context states, which the device carries through the macroblock loop);
    // 8 adds RD refinement of the chosen type's vectors and intra modes in I and P slices (i_mbrd 2: x264_me_refine_qpel_rd, intra_rd_refine; B slices
    // analyse one level down, i.e. as at subme 7): on the device in CABAC sessions under --me hex / umh.  9 adds the refinement in B slices (per-list
    // x264_me_refine_qpel_rd, x264_me_refine_bidir_rd, intra_rd_refine), chroma in their sub-pel costs and the deblock-aware RD costs.  10 and 11 (QP-RD,
    // full-RD trellis) are not implemented.  The highest level whose behaviour IS implemented is reported back
    // With X264GPU_QP_RD=1, 10 (QP-RD, i_mbrd 3: the quantisers around a decided macroblock's own, on RD cost) runs on the device in CABAC sessions under --me hex /
    // umh with --trellis 2 and AQ (the last two are x264's own conditions); whether it does is settled in quantisers(), once AQ is — until then the session is a subme 9 one
    if (env.qp_rd && p.analyse.i_subpel_refine > 9) {
        if (p.analyse.i_subpel_refine > 10) xlog(&p, X264_LOG_INFO, "subme %d: full RD without early termination (the level above 10) is not built: subme 10\n", p.analyse.i_subpel_refine);
        const char *missing = !p.b_cabac ? "CABAC" : p.analyse.i_me_method != X264_ME_HEX && p.analyse.i_me_method != X264_ME_UMH ? "me hex / umh" : nullptr;
        if (missing) xlog(&p, X264_LOG_WARNING, "subme 10 (QP-RD) needs %s in the MI355X path: subme 9\n", missing);
        else qprd_asked = true;
        p.analyse.i_subpel_refine = 9;
    }
    if (p.analyse.i_subpel_refine > 9) { xlog(&p, X264_LOG_WARNING, "subme %d: QP-RD / full-RD trellis of the levels above 9 are not implemented yet: subme 9\n", p.analyse.i_subpel_refine); p.analyse.i_subpel_refine = 9; }
    if (p.analyse.i_subpel_refine >= 8 && (!p.b_cabac || (p.analyse.i_me_method != X264_ME_HEX && p.analyse.i_me_method != X264_ME_UMH))) {
        xlog(&p, X264_LOG_WARNING, "subme %d (RD refinement) needs CABAC and me hex / umh in the MI355X path: subme 7\n", p.analyse.i_subpel_refine); p.analyse.i_subpel_refine = 7;
    }
    p.analyse.i_subpel_refine = clampi(p.analyse.i_subpel_refine, 0, 9);
    // trellis 1 = the final encode of every macroblock quantised by x264's trellis search on the slice's CABAC state: on the device where that state
    // lives, i.e. in CABAC sessions with RD (subme >= 6); trellis 2 = also the block encodes of the intra analysis and every RD candidate
    const int trellis_asked = p.analyse.i_trellis;
    if (p.analyse.i_trellis && (!p.b_cabac || p.analyse.i_subpel_refine < 6)) {
        xlog(&p, X264_LOG_WARNING, "trellis %d needs CABAC and subme >= 6 in the MI355X path (the search reads the CABAC state the device carries for RD): trellis 0\n", p.analyse.i_trellis);
        p.analyse.i_trellis = 0;
    }
    nr_any = NoiseReduction::check_toolset(p, env.nr_any);          // --nr: inter residuals denoised in the macroblock loop (host/noisereduction.hpp); the toolset's share of its rules; psy-trellis gives way to it once the session's mode has passed too (quantisers())
    p.analyse.b_psy = p.analyse.b_psy != 0;
    if (!p.analyse.b_psy) { p.analyse.f_psy_rd = 0; p.analyse.f_psy_trellis = 0; }       // x264 validate_parameters
    p.analyse.f_psy_rd = p.analyse.f_psy_rd < 0 ? 0 : p.analyse.f_psy_rd > 10 ? 10 : p.analyse.f_psy_rd;
    // psy-trellis (--psy-rd a:b, tune film / grain / stillimage): the search's distortion term that rewards keeping the source's energy, in every luma
    // trellis site on the device.  x264 drops it silently without psy or trellis; here it also needs what the device's psy search is built for
    p.analyse.f_psy_trellis = p.analyse.f_psy_trellis < 0 ? 0 : p.analyse.f_psy_trellis > 10 ? 10 : p.analyse.f_psy_trellis;
    if (!trellis_asked) p.analyse.f_psy_trellis = 0;
    if (p.analyse.f_psy_trellis > 0) {
        const char *missing = !p.b_cabac ? "CABAC" : p.analyse.i_subpel_refine < 6 ? "subme >= 6" :
                              p.analyse.i_me_method != X264_ME_HEX && p.analyse.i_me_method != X264_ME_UMH ? "me hex / umh" : nullptr;
        if (missing) { xlog(&p, X264_LOG_WARNING, "psy-trellis needs %s in the MI355X path (the psy search is built for CABAC trellis sessions under me hex / umh): psy-trellis 0\n", missing); p.analyse.f_psy_trellis = 0; }
    }
    // psy RD raises luma quality at chroma's cost, so x264 lowers the chroma quantiser offset to compensate (encoder.c, validate / mb init)
    int eff_chroma_qp_offset = p.analyse.i_chroma_qp_offset;
    if (psy_rd_q8(p)) eff_chroma_qp_offset -= p.analyse.f_psy_rd < 0.25f ? 1 : 2;
    cqo_without_psy_trellis = clampi(eff_chroma_qp_offset, -12, 12);
    if (psy_trellis_q8(p)) eff_chroma_qp_offset -= p.analyse.f_psy_trellis < 0.25f ? 1 : 2;
    eff_chroma_qp_offset = clampi(eff_chroma_qp_offset, -12, 12);
    p.analyse.i_chroma_qp_offset = eff_chroma_qp_offset;          // x264 changes the parameter in place too: the PPS carries it
    p.analyse.b_fast_pskip = p.analyse.b_fast_pskip != 0;
    p.analyse.b_chroma_me = p.analyse.b_chroma_me != 0;
    if (p.b_interlaced) { xlog(&p, X264_LOG_WARNING, "interlaced coding is not implemented in the MI355X path: progressive\n"); p.b_interlaced = 0; }
    if (p.b_constrained_intra) { xlog(&p, X264_LOG_WARNING, "constrained-intra is not implemented in the MI355X path: off\n"); p.b_constrained_intra = 0; }
    if (p.b_intra_refresh) { xlog(&p, X264_LOG_WARNING, "intra-refresh is not implemented in the MI355X path: off\n"); p.b_intra_refresh = 0; }
    // --sliced-threads / --tune zerolatency: i_threads is the number of slices per picture (x264 validate_parameters: at most one per four
    // macroblock rows; auto = as many as that allows, where x264 would count host cores) and there is one GOP in flight
    slices = 1;
    if (p.b_sliced_threads) {
        const int max_slices = mbh / 4 > 1 ? mbh / 4 : 1;
        slices = p.i_threads <= 0 ? max_slices : p.i_threads < max_slices ? p.i_threads : max_slices;
        if (p.i_threads > 0 && slices != p.i_threads) xlog(&p, X264_LOG_INFO, "sliced threads %d -> %d (four macroblock rows per slice)\n", p.i_threads, slices);
        p.i_threads = 1;
        if (slices < 2) p.b_sliced_threads = 0;
        // x264 has no word for "slice threads AND several GOPs in flight"; this library can do both (slices x GOP slots wavefronts per stream).
        // X264GPU_GOP_SLOTS=G asks for it: the --threads G mode (fixed keyint, delay (G-1) x keyint) with every picture in slices
        if (env.gop_slots > 1) p.i_threads = env.gop_slots;
        if (p.i_slice_count > 1) xlog(&p, X264_LOG_INFO, "slices %d ignored under slice threads (%d slices)\n", p.i_slice_count, slices);
        if (slices > 1) p.i_slice_count = 0;
    }
    // --slices N (x264 slices_write: slice i ends at macroblock row (mbh * (i + 1) + N / 2) / N, the split slice threads use too; validate_parameters
    // clips N to the macroblock rows): every slice a wavefront of its own here, which is what makes one stream faster without any delay.
    // Unlike slice threads the loop filter crosses the boundaries (disable_deblocking_filter_idc 0).
    if (!p.b_sliced_threads && p.i_slice_count > 1) {
        p.i_slice_count = p.i_slice_count < mbh ? p.i_slice_count : mbh;
        slices = p.i_slice_count; slices_plain = slices > 1;
    } else if (!p.b_sliced_threads) p.i_slice_count = 0;
    p.i_threads = clampi(p.i_threads, 1, 256);                 // --threads G: GOPs coded in lock-step (1 = no delay)
}

// VBV: x264 validate_parameters' rules for --vbv-maxrate / --vbv-bufsize / --vbv-init / --nal-hrd, and which sessions run it here (single-pass CRF / ABR, one
// picture at a time on the DPB model).  Leaves the effective values in the parameters and `vbv`; runs before the picture structure is settled
void Settings::vbv_rules(x264_param_t &p)
{
    vbv = false;
    if (p.rc.i_vbv_max_bitrate > 0 || p.rc.i_vbv_buffer_size > 0) {
        // (sessions that end up at a constant quantiser: quantisers() maps CRF below 1 and ABR without a bitrate to it)
        const bool cqp = p.rc.i_rc_method == X264_RC_CQP || (p.rc.i_rc_method == X264_RC_CRF && p.rc.f_rf_constant < 1.0f) || (p.rc.i_rc_method == X264_RC_ABR && p.rc.i_bitrate <= 0);
        const char *why = p.i_threads > 1 ? "threads 1 (GOP slots are coded in lock-step, before the sizes of the pictures in front of them are known)" :
                          env.batch >= 2 ? "a session of its own (X264GPU_BATCH codes the sessions of a group in lock-step)" :
                          p.rc.b_stat_read ? "a single pass (the second pass' VBV plan, x264's vbv_pass2, is not implemented)" : nullptr;
        if (cqp) xlog(&p, X264_LOG_WARNING, "VBV is incompatible with constant QP, ignored.\n");
        else if (why) xlog(&p, X264_LOG_WARNING, "VBV (vbv-maxrate / vbv-bufsize) needs %s in the MI355X path: unconstrained\n", why);
        else {
            const bool is_abr = p.rc.i_rc_method == X264_RC_ABR;
            if (p.rc.i_vbv_buffer_size > 0 && p.rc.i_vbv_max_bitrate <= 0) {
                if (is_abr) { xlog(&p, X264_LOG_WARNING, "VBV maxrate unspecified, assuming CBR\n"); p.rc.i_vbv_max_bitrate = p.rc.i_bitrate; }
                else { xlog(&p, X264_LOG_WARNING, "VBV bufsize set but maxrate unspecified, ignored\n"); p.rc.i_vbv_buffer_size = 0; }
            } else if (p.rc.i_vbv_max_bitrate > 0 && p.rc.i_vbv_buffer_size <= 0) { xlog(&p, X264_LOG_WARNING, "VBV maxrate specified, but no bufsize, ignored\n"); p.rc.i_vbv_max_bitrate = 0; }
            if (p.rc.i_vbv_max_bitrate > 0 && p.rc.i_vbv_buffer_size > 0) {
                if (is_abr && p.rc.i_vbv_max_bitrate < p.rc.i_bitrate) { xlog(&p, X264_LOG_WARNING, "max bitrate less than average bitrate, assuming CBR\n"); p.rc.i_bitrate = p.rc.i_vbv_max_bitrate; }
                // x264_ratecontrol_init_reconfigurable: at least one picture's worth of buffer; --vbv-init above 1 is kbit, and the buffer starts with at least one picture's arrival
                const double fps = p.i_fps_num ? (double)p.i_fps_num / p.i_fps_den : 25.0;
                if (p.rc.i_vbv_buffer_size < (int)(p.rc.i_vbv_max_bitrate / fps)) {
                    p.rc.i_vbv_buffer_size = (int)(p.rc.i_vbv_max_bitrate / fps);
                    xlog(&p, X264_LOG_WARNING, "VBV buffer size cannot be smaller than one frame, using %d kbit\n", p.rc.i_vbv_buffer_size);
                }
                auto clipf = [](float v, float lo, float hi) { return v < lo ? lo : v > hi ? hi : v; };
                if (p.rc.f_vbv_buffer_init > 1.f) p.rc.f_vbv_buffer_init = clipf(p.rc.f_vbv_buffer_init / p.rc.i_vbv_buffer_size, 0.f, 1.f);
                const float one = (float)((p.rc.i_vbv_max_bitrate * 1000.0 / fps) / (p.rc.i_vbv_buffer_size * 1000.0));
                p.rc.f_vbv_buffer_init = clipf(p.rc.f_vbv_buffer_init > one ? p.rc.f_vbv_buffer_init : one, 0.f, 1.f);
                vbv = true;
            }
        }
    }
    if (!vbv) { p.rc.i_vbv_max_bitrate = 0; p.rc.i_vbv_buffer_size = 0; }
    p.i_nal_hrd = clampi(p.i_nal_hrd, X264_NAL_HRD_NONE, X264_NAL_HRD_CBR);
    if (p.i_nal_hrd && !vbv) { xlog(&p, X264_LOG_WARNING, "NAL HRD parameters require VBV parameters\n"); p.i_nal_hrd = X264_NAL_HRD_NONE; }
    if (p.i_nal_hrd == X264_NAL_HRD_CBR && (p.rc.i_rc_method != X264_RC_ABR || p.rc.i_vbv_max_bitrate != p.rc.i_bitrate)) {
        xlog(&p, X264_LOG_WARNING, "CBR HRD requires constant bitrate\n"); p.i_nal_hrd = X264_NAL_HRD_VBR;
    }
}

// picture structure: B pictures, --weightp, and whether the session runs on the DPB model or in a batch
void Settings::modes(x264_param_t &p, int &batch_want)
{
    if (p.i_bframe) {
        // (below --subme 7 x264 analyses B slices without RD: k_mb_b.inc's NORD flow; from 7 up their RD decisions count CABAC sizes or CAVLC bits)
        // (--threads G: closed GOPs in lock-step carry B pictures when every GOP has the same picture structure and quantisers: constant quantiser)
        const char *why = (p.i_threads > 1 && p.rc.i_rc_method != X264_RC_CQP && !slots_rc) ? "threads 1, or a constant quantiser with --threads G" : p.i_keyint_max < 2 ? "keyint > 1" :
                          (p.rc.i_rc_method == X264_RC_ABR && p.rc.i_bitrate <= 0) ? "constant-quantiser, CRF or ABR rate control with a bitrate" : nullptr;
        if (why) { xlog(&p, X264_LOG_WARNING, "B-frames need %s in the MI355X path: bframes 0\n", why); p.i_bframe = 0; }
    }
    if (p.i_bframe && p.i_threads > 1) {
        if (p.i_bframe_adaptive) { xlog(&p, X264_LOG_INFO, "b-adapt needs threads 1 (GOPs in lock-step have a fixed structure): b-adapt 0\n"); p.i_bframe_adaptive = 0; }
        if (p.analyse.i_direct_mv_pred == 3) { xlog(&p, X264_LOG_INFO, "direct auto needs threads 1 (its choice follows the pictures coded before, across GOPs): spatial\n"); p.analyse.i_direct_mv_pred = 1; }
    }
    if (p.i_bframe) {
        p.i_bframe_adaptive = clampi(p.i_bframe_adaptive, 0, 2);
        if (p.i_bframe_pyramid == 1) { xlog(&p, X264_LOG_INFO, "b-pyramid strict -> normal\n"); p.i_bframe_pyramid = 2; }
        if (p.i_bframe < 2) p.i_bframe_pyramid = 0;
        if (p.b_open_gop) { xlog(&p, X264_LOG_WARNING, "open-gop is not implemented in the MI355X path: closed GOPs\n"); p.b_open_gop = 0; }
        if (p.analyse.i_direct_mv_pred < 1 || p.analyse.i_direct_mv_pred > 3) { xlog(&p, X264_LOG_INFO, "direct %d -> spatial (B macroblocks without direct prediction are not in the MI355X path)\n", p.analyse.i_direct_mv_pred); p.analyse.i_direct_mv_pred = 1; }
        // (temporal direct prediction is a flag a stream of the group's encoder; auto's choice needs the probe counts read back behind every B picture, which would serialise queued rounds)
        if (p.analyse.i_direct_mv_pred == 3 && env.batch_set) { xlog(&p, X264_LOG_INFO, "direct auto: not in cross-session batches (its choice waits for every B picture's probe counts): spatial\n"); p.analyse.i_direct_mv_pred = 1; }
    } else { p.i_bframe_pyramid = 0; p.analyse.b_weighted_bipred = 0; }
    bframes = p.i_bframe; bpyramid = p.i_bframe_pyramid ? 1 : 0;
    direct_mode = p.i_bframe ? p.analyse.i_direct_mv_pred : 1;
    if (p.i_keyint_max <= 0) p.i_keyint_max = 1;
    if (p.analyse.i_weighted_pred == X264_WEIGHTP_SIMPLE && !bframes) { xlog(&p, X264_LOG_INFO, "weightp 1 (weights for fades, no duplicate references) runs in sessions with B pictures only: weightp 0\n"); p.analyse.i_weighted_pred = X264_WEIGHTP_NONE; }
    if (p.analyse.i_weighted_pred == X264_WEIGHTP_SMART && !bframes) {
        // without B pictures the session can still run on the DPB model, if nothing of the other path is asked for
        const bool tree = p.rc.b_mb_tree && p.rc.i_rc_method != X264_RC_CQP && p.rc.i_lookahead > 0;
        const char *why = p.i_threads > 1 ? "threads 1" : tree ? "no mbtree" :
                          (p.rc.i_rc_method == X264_RC_ABR && p.rc.i_bitrate <= 0) ? "constant-quantiser, CRF or ABR rate control with a bitrate" : p.i_keyint_max < 2 ? "keyint > 1" : nullptr;
        if (why) { xlog(&p, X264_LOG_WARNING, "weightp 2 without B-frames needs %s in the MI355X path: weightp 0\n", why); p.analyse.i_weighted_pred = X264_WEIGHTP_NONE; }
    }
    if (p.analyse.i_weighted_pred == X264_WEIGHTP_SMART && p.i_frame_reference < 2) p.analyse.i_weighted_pred = X264_WEIGHTP_NONE;      // a duplicate needs two references (x264: never placed)
    weightp = p.analyse.i_weighted_pred;
    dpbmode = bframes > 0 || weightp == X264_WEIGHTP_SMART || vbv;          // (VBV: the path that codes one picture at a time and can code it again)
    // --nr on the extended toolset: on the DPB model as a VBV session is, B pictures or not (the presets without them, --tune zerolatency); what that model switches
    // off for a session without B pictures stays off.  (--threads G and all-intra sessions are left to check_modes(), which refuses them as ever)
    if (nr_any && p.analyse.i_noise_reduction && p.i_threads <= 1 && p.i_keyint_max >= 2) dpbmode = true;
    if (env.batch >= 2) {
        // cross-session batcher: this session joins (or starts) a group of N sessions coded in lock-step, if its picture structure is fixed
        // (macroblock-tree, --aq-mode 2 / 3 and --direct temporal leave every picture's type alone: the member's lookahead runs them, the group carries what it decides)
        const char *why = p.i_threads > 1 ? "threads 1" : slices > 1 || p.b_sliced_threads ? "one slice per picture" : p.i_scenecut_threshold > 0 ? "scenecut 0" :
                          (bframes && p.i_bframe_adaptive) ? "b-adapt 0" : p.rc.i_rc_method == X264_RC_ABR ? "constant-quantiser or CRF rate control" : nullptr;
        if (why) xlog(&p, X264_LOG_WARNING, "X264GPU_BATCH needs %s (picture k must have the same type in every session of a batch): this session runs on its own\n", why);
        else { batch_want = env.batch; dpbmode = true; }
    }
    if (dpbmode && !bframes) { p.rc.b_mb_tree = 0; }
    if (weightp) xlog(&p, X264_LOG_INFO, "weightp %d: weights for fades from the lookahead (luma, and the chroma planes beside it)%s\n", weightp, weightp == X264_WEIGHTP_SMART ? ", duplicates of reference 0 on every P picture" : "");
    keyint = p.i_keyint_max;
}

// rate control: which method the session really runs (passes of a 2-pass encode, zones, AQ, macroblock-tree), the quantisers, profile and level, the DPB model
void Settings::quantisers(x264_param_t &p, RateControl &rc, Dpb &dpb, MbTreeStats &tstats)
{
    // rate control: constant QP (X264_RC_CQP, codec.c:1498-1502) and single-pass CRF without AQ / mbtree (codec.c:1504-1507, the
    // driver's default session) when one GOP is in flight; ABR and CRF under --threads > 1 map to their nominal quantiser
    int qp = p.rc.i_rc_method == X264_RC_CQP ? p.rc.i_qp_constant : p.rc.i_rc_method == X264_RC_CRF ? (int)(p.rc.f_rf_constant + 0.5f) : 26;
    rc.crf = p.rc.i_rc_method == X264_RC_CRF && p.rc.f_rf_constant >= 1.0f;       // also under --threads G: its quantisers follow from the lookahead costs alone
    // 2-pass: the second pass plans every picture's quantiser from the first pass' statistics; sessions on the DPB model (B pictures or --weightp 2)
    rc.pass2 = p.rc.b_stat_read && p.rc.i_rc_method == X264_RC_ABR && p.rc.i_bitrate > 0 && p.i_threads <= 1 && dpbmode && p.rc.psz_stat_in && !env.batch_set;
    rc.pass1 = p.rc.b_stat_write && !p.rc.b_stat_read && p.i_threads <= 1 && dpbmode && p.rc.psz_stat_out && !env.batch_set;
    if ((p.rc.b_stat_read && !rc.pass2) || (p.rc.b_stat_write && !p.rc.b_stat_read && !rc.pass1)) {
        // a pass whose statistics cannot be honoured keeps its rate control: it runs as the single-pass session of the same method (ABR at i_bitrate
        // for the driver's multipass encodes, codec.c:1509-1527), as every pass did before 2-pass existed here — not at a constant quantiser
        xlog(&p, X264_LOG_WARNING, "2-pass statistics need threads 1 and B-frames or weightp 2 (the DPB-model path) in the MI355X path: this pass runs as a single pass without them\n");
        if (!rc.pass2) p.rc.b_stat_read = 0;
        if (!rc.pass1) p.rc.b_stat_write = 0;
    }
    rc.abr = p.rc.i_rc_method == X264_RC_ABR && p.i_threads <= 1 && p.rc.i_bitrate > 0 && !p.rc.b_stat_read;      // single pass, no VBV
    if (p.rc.b_stat_write && p.rc.b_stat_read && !rc.pass2) xlog(&p, X264_LOG_INFO, "this pass runs without the statistics: they stay as the first pass wrote them\n");
    if (p.rc.i_rc_method != X264_RC_CQP && !rc.by_cost() && !rc.pass2) xlog(&p, X264_LOG_WARNING, "this rate control mode is not implemented yet (ABR with --threads > 1): constant qp %d\n", qp);
    if (qp < 1) { xlog(&p, X264_LOG_WARNING, "lossless is not supported: qp 1\n"); qp = 1; }
    if (!rc.by_cost() && !rc.pass2) p.rc.i_rc_method = X264_RC_CQP;
    if ((rc.pass1 || rc.pass2) && p.rc.b_mb_tree) {
        if (!env.mbtree_stats) { xlog(&p, X264_LOG_INFO, "2-pass: the macroblock-tree statistics file is not implemented in the MI355X path: mbtree 0 in both passes\n"); p.rc.b_mb_tree = 0; }
        else if (rc.pass2) {
            // the second pass has no future pictures: no lookahead, no tree of its own — kept pictures take the offsets the first pass' tree left in <stats>.mbtree,
            // the plan takes the tree's RCEQ.  The session is set up as the tree-less one (rc-lookahead 0) and reports mbtree 1 (x264_encoder_open, once every part is open).
            // Needs what 2-pass needs (threads 1, the DPB-model path, no X264GPU_BATCH: rc.pass2 says so); VBV and zones in a second pass stay as they are
            tstats.reading = rc.tree_read = tstats.check_read(p, p.rc.psz_stat_in, nmb);
            p.rc.b_mb_tree = 0;
        }
        // (a first pass keeps its tree: the single-pass CRF / ABR + tree session plus the statistics; whether the tree really runs is settled below)
    }
    rc.parse_zones(p);
    if (!rc.zones.empty()) xlog(&p, X264_LOG_INFO, "%d zone%s (quantiser / bitrate factor per range of pictures)\n", (int)rc.zones.size(), rc.zones.size() > 1 ? "s" : "");
    if (!rc.zones.empty() && rc.pass2) xlog(&p, X264_LOG_WARNING, "zones are not applied to the second pass' plan in the MI355X path (the first pass and single-pass sessions honour them)\n");
    if (vbv && (!rc.by_cost() || rc.pass2)) {          // (vbv_rules() admitted a session whose rate control fell back since)
        xlog(&p, X264_LOG_WARNING, "VBV is incompatible with constant QP, ignored.\n");
        vbv = false; p.rc.i_vbv_max_bitrate = 0; p.rc.i_vbv_buffer_size = 0; p.i_nal_hrd = X264_NAL_HRD_NONE;
    }
    rc.vbv = vbv; rc.filler = vbv && p.i_nal_hrd == X264_NAL_HRD_CBR;
    NoiseReduction::check_modes(p, dpbmode);
    if (!p.analyse.i_noise_reduction) nr_any = false;
    if (nr_any) xlog(&p, X264_LOG_INFO, "nr %d runs on the extended toolset (X264GPU_NR_ANY: the denoising kernels of every inter toolset, the session on the DPB model)\n", p.analyse.i_noise_reduction);
    if (p.analyse.i_noise_reduction && p.analyse.f_psy_trellis > 0) {
        // nr runs (toolset and mode have passed; from here on only a device failure stops it, and that fails the open): psy-trellis gives way, with its share of the
        // chroma quantiser offset (the macroblock loop has psy instantiations and denoising instantiations, none with both: the build would double again)
        xlog(&p, X264_LOG_WARNING, "psy-trellis is not run beside noise reduction in the MI355X path (nr %d wins): psy-trellis 0\n", p.analyse.i_noise_reduction);
        p.analyse.f_psy_trellis = 0; p.analyse.i_chroma_qp_offset = cqo_without_psy_trellis;
    }
    if (p.i_slice_max_size > 0 || p.i_slice_max_mbs > 0) { xlog(&p, X264_LOG_WARNING, "slice-max-size / slice-max-mbs are not implemented in the MI355X path (slices are cut by --slices N or slice threads only)\n"); p.i_slice_max_size = p.i_slice_max_mbs = 0; }
    if (p.b_fake_interlaced || p.b_pic_struct) { xlog(&p, X264_LOG_WARNING, "fake-interlaced / pic-struct are not implemented in the MI355X path: off\n"); p.b_fake_interlaced = p.b_pic_struct = 0; }
    if (p.b_bluray_compat) { xlog(&p, X264_LOG_WARNING, "bluray-compat is not implemented in the MI355X path: off\n"); p.b_bluray_compat = 0; }
    // adaptive quantisation: variance AQ (mode 1) under CRF / ABR; x264 itself switches AQ off under constant QP and at strength 0
    if (p.rc.i_rc_method == X264_RC_CQP || p.rc.f_aq_strength <= 0) p.rc.i_aq_mode = X264_AQ_NONE;
    // macroblock-tree: needs a rate-controlled session and pictures held back (rc-lookahead); x264 switches it off under constant QP
    if (p.rc.i_rc_method == X264_RC_CQP || p.rc.i_lookahead <= 0) p.rc.b_mb_tree = 0;
    if (p.rc.b_mb_tree && p.i_threads > 1 && !slots_rc) { xlog(&p, X264_LOG_INFO, "mbtree needs threads 1 (GOPs in lock-step are coded before what follows them is seen): mbtree 0\n"); p.rc.b_mb_tree = 0; }
    p.rc.b_mb_tree = p.rc.b_mb_tree != 0;
    tstats.writing = rc.tree_write = rc.pass1 && p.rc.b_mb_tree && env.mbtree_stats;
    // (VBV plans over the lookahead too, with or without the tree: x264's vbv_lookahead; rc-lookahead 0 leaves it the reactive algorithm)
    { const int cap = p.i_keyint_max < 250 ? (p.i_keyint_max > 1 ? p.i_keyint_max : 1) : 250;
      p.rc.i_lookahead = p.rc.b_mb_tree ? clampi(p.rc.i_lookahead, 1, cap) : vbv ? clampi(p.rc.i_lookahead, 0, cap) : 0; }
    p.rc.i_aq_mode = clampi(p.rc.i_aq_mode, 0, 3);
    if (p.rc.i_aq_mode > X264_AQ_VARIANCE && !dpbmode) {
        xlog(&p, X264_LOG_WARNING, "aq-mode %d needs B-frames or weightp 2 (the DPB-model path) in the MI355X path: aq-mode 1\n", p.rc.i_aq_mode); p.rc.i_aq_mode = X264_AQ_VARIANCE;
    }
    aq_mode = p.rc.i_aq_mode;
    p.rc.i_qp_constant = clampi(qp, 1, 51);
    p.rc.i_qp_min = clampi(p.rc.i_qp_min, 1, 51); p.rc.i_qp_max = clampi(p.rc.i_qp_max, p.rc.i_qp_min, 51);
    if (qprd_asked) {
        // --subme 10 under X264GPU_QP_RD=1 (toolset() left the session at subme 9): x264's own rule first, then what the device's QP-RD kernels are not built beside
        if (p.analyse.i_trellis != 2 || !p.rc.i_aq_mode) xlog(&p, X264_LOG_WARNING, "subme 10 (QP-RD) requires trellis 2 and aq-mode > 0, as in x264 (%s missing): subme 9\n", p.analyse.i_trellis != 2 ? p.rc.i_aq_mode ? "trellis 2" : "both" : "aq-mode > 0");
        else if (p.analyse.i_noise_reduction || p.analyse.f_psy_trellis > 0) xlog(&p, X264_LOG_INFO, "subme 10: QP-RD is not run beside %s in the MI355X path (%s keeps its kernels): subme 9\n", p.analyse.i_noise_reduction ? "noise reduction" : "psy-trellis", p.analyse.i_noise_reduction ? "nr" : "psy-trellis");
        else { qp_rd = true; p.analyse.i_subpel_refine = 10; }
    }
    if (p.i_threads > 1 && p.i_scenecut_threshold) { xlog(&p, X264_LOG_INFO, "scenecut needs threads 1 (GOPs in lock-step have a fixed structure): scenecut 0\n"); p.i_scenecut_threshold = 0; }
    // x264 validate_parameters: min-keyint auto = min(keyint / 10, fps), then [1, keyint / 2 + 1]
    if (p.i_keyint_min <= 0) { const int fps = (int)(p.i_fps_num / (p.i_fps_den ? p.i_fps_den : 1)); p.i_keyint_min = p.i_keyint_max / 10 < fps ? p.i_keyint_max / 10 : fps; }
    p.i_keyint_min = clampi(p.i_keyint_min, 1, p.i_keyint_max / 2 + 1);
    keyint_min = p.i_keyint_min;
    qp_p = p.rc.i_qp_constant;
    qp_i = clampi((int)(qp_p - 6.0 * log2(p.rc.f_ip_factor > 0 ? p.rc.f_ip_factor : 1.0) + 0.5), 1, 51);
    pic_init_qp = rc.by_cost() ? 26 : clampi(qp_p, 0, 51);          // CRF moves the slice quantiser both ways: centre the +-26 range of slice_qp_delta
    profile_idc = p.analyse.b_transform_8x8 ? 100 : p.b_cabac ? 77 : 66;        // High for the 8x8 transform, Main for CABAC alone, else Baseline-compatible
    level_idc = p.i_level_idc > 0 ? p.i_level_idc : pick_level(&p, nmb, p.i_frame_reference);
    p.i_level_idc = level_idc;
    log2_max_frame_num = 4;
    {   // x264 sps init: max_frame_num = keyint * (1 + b-pyramid) + 1
        const long max_frame_num = (long)(keyint < 65536 ? keyint : 65535) * (bpyramid + 1) + 1;
        while ((1L << log2_max_frame_num) <= max_frame_num && log2_max_frame_num < 16) log2_max_frame_num++;
    }
    if (weightp && profile_idc == 66) profile_idc = 77;                  // explicit weighted prediction is a Main profile tool
    if (dpbmode) {
        // x264 sps init: pic_order_cnt_type 0 with room for the largest POC distance of a mini-GOP (type 2 without B pictures); the DPB model owns
        // frame_num / lists / marking
        dpb.configure(p.i_frame_reference, bframes, bpyramid, log2_max_frame_num, weightp);
        const int max_delta_poc = (bframes + 2) * (bpyramid + 1) * 2;
        log2_max_poc_lsb = bframes ? 4 : 0;
        while (bframes && (1 << log2_max_poc_lsb) <= max_delta_poc * 2) log2_max_poc_lsb++;
        level_idc = p.i_level_idc > 0 ? p.i_level_idc : pick_level(&p, nmb, dpb.max_dpb);
        p.i_level_idc = level_idc;
    }
    if (vbv && p.i_nal_hrd) {
        // x264_ratecontrol_init_reconfigurable, "Init HRD": rate and size in the value / scale notation (the VBV then runs on what the notation keeps of them), the
        // lengths of the delay fields from the longest delays the session can produce (a buffering period is at most keyint pictures long, "arbitrary" MAX_DURATION 0.5 s
        // a picture — and never shorter than the two ticks a picture that constant-frame-rate pictures really take)
        HrdParams &hr = hrd;
        const int rate = p.rc.i_vbv_max_bitrate * 1000, size = p.rc.i_vbv_buffer_size * 1000;
        hr.present = 1; hr.cbr = p.i_nal_hrd == X264_NAL_HRD_CBR;
        hr.bit_rate_scale = clampi(__builtin_ctz((unsigned)rate) - 6, 0, 15); hr.bit_rate_value = rate >> (hr.bit_rate_scale + 6); hr.bit_rate_unscaled = hr.bit_rate_value << (hr.bit_rate_scale + 6);
        hr.cpb_size_scale = clampi(__builtin_ctz((unsigned)size) - 4, 0, 15); hr.cpb_size_value = size >> (hr.cpb_size_scale + 4); hr.cpb_size_unscaled = hr.cpb_size_value << (hr.cpb_size_scale + 4);
        const double ticks = 0.5 * (double)(p.i_timebase_den * 2) / p.i_timebase_num;
        double max_cpb = p.i_keyint_max * ticks; if (max_cpb < 2.0 * p.i_keyint_max) max_cpb = 2.0 * p.i_keyint_max;
        double max_dpb = dpb.max_dpb * ticks; if (max_dpb < 2.0 * (dpb.num_reorder + bframes + 2)) max_dpb = 2.0 * (dpb.num_reorder + bframes + 2);
        const int max_cpb_output_delay = max_cpb < (double)INT_MAX ? (int)max_cpb : INT_MAX, max_dpb_output_delay = max_dpb < (double)INT_MAX ? (int)max_dpb : INT_MAX;
        const int max_delay = (int)(90000.0 * (double)hr.cpb_size_unscaled / hr.bit_rate_unscaled + 0.5);
        auto bits = [](int v) { return v > 0 ? 32 - __builtin_clz((unsigned)v) : 0; };
        hr.initial_cpb_removal_delay_length = 2 + clampi(bits(max_delay), 4, 22);
        hr.cpb_removal_delay_length = clampi(bits(max_cpb_output_delay), 4, 31);
        hr.dpb_output_delay_length = clampi(bits(max_dpb_output_delay), 4, 31);
        rc.hrd_rate = hr.bit_rate_unscaled; rc.hrd_size = hr.cpb_size_unscaled;
        if (hr.bit_rate_value < 1 || hr.cpb_size_value < 1) { xlog(&p, X264_LOG_WARNING, "nal-hrd: rate or size too small for the HRD's notation: none\n"); hr = HrdParams(); p.i_nal_hrd = X264_NAL_HRD_NONE; rc.hrd_rate = rc.hrd_size = 0; rc.filler = false; }
    }
}

// the GOP-slot count, --mvrange and the pictures of the session in flight
void Settings::in_flight(x264_param_t &p, const RateControl &rc, Dpb &dpb, int batch_want)
{
    // (quantisers planned ahead: a ring picture has up to three rows of the plan store beside it)
    G = GopSlots::fit(p, keyint, slots_rc ? 3 * (size_t)nmb * 4 : 0);
    if (G <= 1) slots_rc = false;          // (nothing to run in parallel: the session is the --threads 1 one)
    // x264 validate_parameters: --mvrange defaults to the level's limit (x264_levels[].mv_range), never above 512 here
    if (p.analyse.i_mv_range <= 0) {
        p.analyse.i_mv_range = 512;
        for (int i = 0; x264_levels[i].level_idc; i++) if (x264_levels[i].level_idc == level_idc) p.analyse.i_mv_range = x264_levels[i].mv_range;
    }
    p.analyse.i_mv_range = clampi(p.analyse.i_mv_range, 32, 512);
    inflight = 1;
    if (p.analyse.i_noise_reduction && dpbmode && p.i_bframe > 0 && env.inflight_set)
        xlog(&p, X264_LOG_INFO, "nr: one picture in flight (X264GPU_INFLIGHT is not used: the session has one noise-reduction state, moved on in coding order)\n");
    if (dpbmode && p.i_bframe > 0 && G == 1 && !batch_want && !rc.reads_sizes() && direct_mode != 3 && !p.analyse.i_noise_reduction) {
        // (--direct auto chooses a B picture's mode from the skip counts of the one before, ABR and 2-pass a picture's quantiser from the sizes of the ones before:
        //  those sessions code one picture at a time)
        const int want = env.dump_records ? 1 : env.inflight_set ? env.inflight : 4,          // (the debugging dump follows the serial path)
                  extra = want - 1 < 7 - dpb.max_dpb ? want - 1 : 7 - dpb.max_dpb;
        if (extra >= 1) { inflight = extra + 1; dpb.extra_slots = extra; }
    }
    if (dpbmode) dpb_slots = dpb.max_dpb + dpb.extra_slots;
}

// whether the session has a lookahead object, how many pictures are held back, the size of the queue's ring
void Settings::lookahead_window(x264_param_t &p, RateControl &rc, const MbTreeStats &tstats)
{
    lookahead_asked = p.rc.i_lookahead;
    // (sessions on the DPB model take scene cuts from x264's own analysis; a second pass over the tree file: the AQ kernel only)
    lookahead = (p.i_scenecut_threshold > 0 && !dpbmode) || rc.by_cost() || aq_mode >= 2 || tstats.reading;
    // lookahead queue: rc-lookahead pictures are held back when the macroblock-tree is on (x264's sync lookahead), none otherwise
    mbtree = p.rc.b_mb_tree && lookahead;
    L = mbtree || vbv ? p.rc.i_lookahead : 0;
    // pictures are held back anyway and the quantisers do not depend on coded sizes: overlap the GPU stage of the next picture with
    // the entropy coding of this one (one more picture of delay); X264GPU_HOST_PIPELINE=0 keeps the two stages in one call
    pipeline = G == 1 && L > 0 && rc.crf && !env.pipeline_off;
    Q = L + 1 + (pipeline ? 1 : 0);
    if (dpbmode) {
        if (L > 60) { rc_lookahead_cut = L; L = 60; p.rc.i_lookahead = 60; }
        pipeline = false; Q = L + 2 * (bframes + 1) + 2;      // the lookahead window + display-order queue + the mini-GOP being coded
    }
    st_wait = bframes > L ? bframes : L;          // x264 i_slicetype_length
    // x264 h->frames.i_delay: the trellis over picture types looks max(bframes, 3) * 4 pictures ahead
    if (dpbmode && bframes && p.i_bframe_adaptive == 2) { const int d = (bframes > 3 ? bframes : 3) * 4; if (d > st_wait) st_wait = d; if (Q < st_wait + 2 * (bframes + 1) + 2) Q = st_wait + 2 * (bframes + 1) + 2; }
    if (dpbmode && inflight > 1) Q += inflight + bframes + 1;           // ... + the pictures in flight (their source pictures and offsets are read when their kernels run)
    if (dpbmode && Q > 128) {          // the lookahead object holds 128 pictures
        window_cut = Q - 128;
        L = L > window_cut ? L - window_cut : 0; p.rc.i_lookahead = L;
        if (st_wait > 128 - 2 * (bframes + 1) - 2) st_wait = 128 - 2 * (bframes + 1) - 2;
        Q = 128;
    }
    rc.vbv_lookahead = vbv && L > 0;
    if (vbv) p.rc.i_lookahead = L;
    aq_strength = aq_mode == X264_AQ_VARIANCE ? p.rc.f_aq_strength * 1.0397f : aq_mode >= 2 ? p.rc.f_aq_strength : 0.f;      // (modes 2 / 3: the plain strength, x264_adaptive_quant_frame scales it by the picture's mean itself)
    tree_strength = 5.0f * (1.0f - p.rc.f_qcompress);
}

void Settings::log_lookahead(const x264_param_t &p) const
{
    if (rc_lookahead_cut) xlog(&p, X264_LOG_INFO, "rc-lookahead %d -> 60 in sessions with B pictures (the lookahead keeps every queued picture's half-resolution planes and searches on the device)\n", rc_lookahead_cut);
    if (window_cut) xlog(&p, X264_LOG_INFO, "lookahead window shortened by %d pictures (128 pictures are held at most)\n", window_cut);
    if (vbv) {
        xlog(&p, X264_LOG_INFO, "VBV: maxrate %d kbit/s, bufsize %d kbit, init %.3f%s; %s; x264's row-level re-quantisation is replaced by picture re-encode: a picture that would under-run the buffer is coded again at a higher quantiser\n",
             p.rc.i_vbv_max_bitrate, p.rc.i_vbv_buffer_size, (double)p.rc.f_vbv_buffer_init, p.i_nal_hrd == X264_NAL_HRD_CBR ? ", nal-hrd cbr" : p.i_nal_hrd ? ", nal-hrd vbr" : "",
             L > 0 ? "quantisers planned over the lookahead" : "rc-lookahead 0: the reactive algorithm");
        if (p.b_vfr_input) xlog(&p, X264_LOG_INFO, "VBV: variable frame rate durations are not implemented in the MI355X path: every picture stays in the buffer for 1 / fps\n");
        if (p.rc.f_rf_constant_max > 0) xlog(&p, X264_LOG_WARNING, "crf-max is not implemented in the MI355X path: ignored\n");
    }
}

x264gpu_config Settings::device_config(const x264_param_t &p) const
{
    x264gpu_config cfg = {};
    cfg.width = p.i_width; cfg.height = p.i_height; cfg.streams = G; cfg.refs = p.i_frame_reference; cfg.slices = slices; cfg.slices_plain = slices_plain; cfg.cabac = p.b_cabac;
    cfg.qp_i = qp_i; cfg.qp_p = qp_p; cfg.me_range = p.analyse.i_me_range; cfg.subme = p.analyse.i_subpel_refine;
    cfg.deblock = p.b_deblocking_filter; cfg.deblock_alpha = p.i_deblocking_filter_alphac0; cfg.deblock_beta = p.i_deblocking_filter_beta;
    cfg.chroma_qp_offset = p.analyse.i_chroma_qp_offset;
    cfg.rd = p.analyse.i_subpel_refine >= 8 ? 63 : p.analyse.i_subpel_refine >= 6; cfg.psy_rd_q8 = psy_rd_q8(p);      // 63: RD + every refinement site (x264's i_mbrd 2)
    if (p.analyse.i_subpel_refine >= 9 && p.b_deblocking_filter) cfg.rd |= 64;          // h->mb.b_deblock_rdo: whole-macroblock RD costs measured after the loop filter
    cfg.psy_trellis_q8 = psy_trellis_q8(p);
    if (qp_rd) { cfg.qp_rd = 1; cfg.qp_min = p.rc.i_qp_min; cfg.qp_max = p.rc.i_qp_max; }          // (x264: rc.i_qp_min .. min(rc.i_qp_max, 51); both clipped to 1 .. 51 in quantisers())
    cfg.trellis = p.analyse.i_trellis == 2 ? 63 + 64 : p.analyse.i_trellis ? 63 : 0;         // every quantiser call of the final encode; + 64: of the analysis too
    cfg.psy = cfg.rd && p.analyse.b_psy;           // x264: the chroma lambda offset table follows b_psy, whatever the psy-rd strength
    cfg.deadzone_inter = p.analyse.i_luma_deadzone[0]; cfg.deadzone_intra = p.analyse.i_luma_deadzone[1];
    cfg.dct_decimate = p.analyse.b_dct_decimate;
    // P slices follow analyse.inter, I slices analyse.intra (bit8 marks the separate I-slice set)
    cfg.partitions = ((p.analyse.inter & X264_ANALYSE_PSUB16x16) ? 1 : 0) | ((p.analyse.inter & X264_ANALYSE_I4x4) ? 2 : 0) | ((p.analyse.inter & X264_ANALYSE_I8x8) ? 4 : 0) |
                     0x100 | ((p.analyse.intra & X264_ANALYSE_I4x4) ? 0x200 : 0) | ((p.analyse.intra & X264_ANALYSE_I8x8) ? 0x400 : 0) |
                     ((p.analyse.inter & X264_ANALYSE_BSUB16x16) ? 0x800 : 0);      // B slices: b8x8
    cfg.dct8x8 = p.analyse.b_transform_8x8;
    cfg.me_method = p.analyse.i_me_method == X264_ME_DIA ? 0 : p.analyse.i_me_method == X264_ME_HEX ? 1 : p.analyse.i_me_method == X264_ME_UMH ? 2 : 3;
    cfg.aq_mode = aq_mode == X264_AQ_VARIANCE; cfg.aq_strength = p.rc.f_aq_strength * 1.0397f;
    cfg.mixed_refs = p.analyse.b_mixed_references && (p.analyse.inter & X264_ANALYSE_PSUB16x16) != 0;
    cfg.chroma_me = p.analyse.b_chroma_me && p.analyse.i_subpel_refine >= 5;     // x264: h->mb.b_chroma_me in P slices
    cfg.fast_pskip = p.analyse.b_fast_pskip;
    cfg.mv_range = p.analyse.i_mv_range;
    if (dpbmode) { cfg.dpb = dpb_slots; cfg.weightb = p.analyse.b_weighted_bipred; }
    return cfg;
}

}  // namespace x264host
